"""-m gpu: dropout of the train passes (include/fsmg.h "Dropout").

Bitwise laws first (the device's masks against the numpy generator, keeps of one against a never-enabled handle in the serial order,
the passes that never drop, the split form, determinism, the pass counter), then every tensor of a dropped pass against the fp64
restatement of tests/dropout_ref.py ELEMENT BY ELEMENT: the families of backward_ref.COMPONENTWISE and SLICEWISE plus 'drop' (the
masked activations of every site) to M = 8 times e32 of the masked fp32 restatement, and exact zeros wherever the scale is zero.  The
masks of the references come from numpy, never from the device.  Measured ratios: tests/COMPONENTWISE_DROPOUT.md.
"""
import os

import numpy as np
import pytest

import backward_ref as R
import dropout_ref as D
import masked_ref as MR
from conftest import small_config
from gpu_utils import f64_params, new_model, rel_max
from oracle import lstm_oracle as O
from test_gpu_componentwise import FUSED, M, device_tensors

pytestmark = pytest.mark.gpu

SEED = 0x0123456789ABCDEF
DROP = dict(keep_input=0.8, keep_output=0.5, variational=False, seed=SEED)
IDX = [1, 3, 5, 8, 9]          # ragged last group of four | two layers | H = 200 padded to 256 | bf16-split chains | pair kernels, stacked
NLL_RTOL = 1e-4                # the project's bound on a loss against fp64
REL_MAX = 5e-4                 # ... and on a tensor after outer updates (tests/test_gpu_msgd.py, test_gpu_parity.py)


def case(idx):
    over, N, K, Q, seed = R.CW_SHAPES[idx]
    cfg = small_config(**over)
    sup, qry = R.episode(cfg, N, K, Q, seed)
    return cfg, sup.astype(np.int32), qry.astype(np.int32), N * (K + Q)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


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


def site_width(cfg, site):
    return cfg['embedding_size'] if site == 0 else cfg['hidden_size']


# ----------------------------------------------------------------------------- (a) (b) (g) the device's masks
@pytest.mark.parametrize('idx', [1, 3, 5])
def test_device_masks_are_the_numpy_masks(idx):
    cfg, sup, qry, B = case(idx)
    T = cfg['max_len']
    model = new_model(cfg, max_sequences=B)
    with pytest.raises(Exception, match='STATE'):
        model.dropout_mask(0, 0, B)
    for variational in (False, True):
        model.dropout_enable(**dict(DROP, variational=variational))
        for p in (0, (1 << 32) + 9):
            for site in range(cfg['n_layers'] + 1):
                keep = D.keep_of(DROP, site)
                got = model.dropout_mask(p, site, B)
                want = D.site_mask(SEED, p, site, T, B, site_width(cfg, site), keep, variational)
                assert got.shape == want.shape and np.array_equal(got, want), (variational, p, site)
                if variational:                       # (g) equal over t
                    assert np.all(got == got[:1])
                else:
                    assert not np.all(got == got[:1])
    assert model.dropout_info()['last_pass'] == -1    # reading masks runs no pass


@pytest.mark.parametrize('idx', [5, 8])
def test_kept_fraction_of_the_device_masks(idx):
    """|kept / n - keep| <= 5 sqrt(keep (1 - keep) / n)"""
    cfg, sup, qry, B = case(idx)
    model = new_model(cfg, max_sequences=B)
    for keep in (0.35, 0.8):
        model.dropout_enable(keep_input=keep, keep_output=keep, seed=SEED + 1)
        for p in (0, 1):
            for site in (0, 1):
                m = model.dropout_mask(p, site, B)
                k = float(np.float32(keep))
                sigma = np.sqrt(k * (1 - k) / m.size)
                print('DROP|kept|%s|keep %.2f|pass %d|site %d|%.2f sigma' % (R.shape_id(R.CW_SHAPES[idx]), keep, p, site, abs(m.mean() - k) / sigma))
                assert abs(m.mean() - k) <= 5 * sigma


# ----------------------------------------------------------------------------- (c) keeps of one
def _two_steps(model, eps):
    losses = [model.train_step(*e) for e in eps]
    return losses, state_of(model)


@pytest.mark.parametrize('shape', [R.CW_SHAPES[3], R.CW_SHAPES[8], R.CW_SHAPES[9], FUSED], ids=R.shape_id)
def test_keeps_of_one_equal_a_never_enabled_handle_in_the_serial_order(shape, monkeypatch):
    """enabled with both keeps 1 the step launches nothing of dropout's and runs the serial order: every output of fsmg_train_step and
    the parameters after it are those of a never-enabled handle created with FSMG_XCD_OVERLAP=0 FSMG_OVERLAP=0.  FUSED is cfg-B at full
    width, where the never-enabled default is the XCD-partitioned order -- and where fsmg_create gives a handle that may take that order
    the bf16-split XCD-local chains at 45 rows (api_handle.hip: the packed chains need them), which the serial handle would not pick by
    itself: the recurrence family stays the enabled handle's, so the serial handle of that shape is created with FSMG_XCD_BX3=1 too."""
    over, N, K, Q, seed = shape
    cfg = small_config(**over)
    B = N * (K + Q)
    eps = [tuple(a.astype(np.int32) for a in R.episode(cfg, N, K, Q, seed + s)) for s in range(2)]
    monkeypatch.setenv('FSMG_XCD_OVERLAP', '0')
    monkeypatch.setenv('FSMG_OVERLAP', '0')
    if shape is FUSED:
        monkeypatch.setenv('FSMG_XCD_BX3', '1')
    plain = new_model(cfg, max_sequences=B)
    want_losses, want = _two_steps(plain, eps)
    plain.close()
    monkeypatch.delenv('FSMG_XCD_BX3', raising=False)
    monkeypatch.delenv('FSMG_XCD_OVERLAP')
    monkeypatch.delenv('FSMG_OVERLAP')
    model = new_model(cfg, max_sequences=B)
    model.dropout_enable(keep_input=1.0, keep_output=1.0, seed=5)
    got_losses, got = _two_steps(model, eps)
    assert model.stats()['timeouts'] == 0 and model.step == 2
    assert [np.float32(x).view(np.uint32) for x in got_losses] == [np.float32(x).view(np.uint32) for x in want_losses]
    same_state(got, want, 'keeps of one')
    assert model.dropout_info()['next_pass'] == 2           # the passes are counted all the same
    with pytest.raises(Exception, match='STATE'):
        model.dropout_read(0, B)                            # ... and no site was written


# ----------------------------------------------------------------------------- (d) the passes that never drop
def test_eval_score_generate_cache_and_maml_eval_never_drop():
    cfg, sup, qry, B = case(3)
    T = cfg['max_len']
    model = new_model(cfg, max_sequences=B)
    songs = np.concatenate([sup.reshape(-1, T), qry.reshape(-1, T)])

    def outputs():
        out = [np.float32(model.eval_step(qry))]
        sc = model.score(songs, rank=True, entropy=True)
        out += [sc['logprob'], sc['entropy'], sc['row_nll']]
        out.append(model.generate(4, 6, seed=11).astype(np.float32))
        cache = model.cache_build(sup.reshape(-1, T), n_groups=sup.shape[0])
        keys, vals = cache.get()
        cache.close()
        out += [keys, vals.astype(np.float32)]
        out.append(np.float32(model.maml_eval(sup, qry, 2, 0.1)))
        return out

    before = outputs()
    model.dropout_enable(**DROP)
    after = outputs()
    info = model.dropout_info()
    assert info['enabled'] and info['last_pass'] == -1 and info['next_pass'] == 0        # not one dropped pass, the adaptation included
    for i, (x, y) in enumerate(zip(before, after)):
        assert np.array_equal(bits(x), bits(y)), i
    model.train_step(sup, qry)                                                            # (the switch is live: a train pass is dropped)
    assert model.dropout_info()['last_pass'] == 0
    model.dropout_disable()
    model.train_step(sup, qry)
    assert model.dropout_info()['next_pass'] == 1 and not model.dropout_info()['enabled']


# ----------------------------------------------------------------------------- (e) (f) split form, determinism, the next pass
@pytest.mark.parametrize('idx', [3, 8])
def test_split_form_same_seed_and_the_next_pass(idx):
    cfg, sup, qry, B = case(idx)
    a, b, c = (new_model(cfg, max_sequences=B) for _ in range(3))
    for m in (a, b, c):
        m.dropout_enable(**DROP)
        m.dropout_set_pass(41)
    la = a.train_step(sup, qry)
    b.forward_backward(sup, qry)
    lb = b.apply_update(1.0)
    assert np.float32(la).view(np.uint32) == np.float32(lb).view(np.uint32)
    same_state(state_of(a), state_of(b), 'split form')
    assert a.dropout_info()['last_pass'] == b.dropout_info()['last_pass'] == 41
    # another pass index: other masks, another loss
    c.dropout_set_pass(42)
    lc = c.train_step(sup, qry)
    assert lc != la and abs(lc - la) > 1e-6 * abs(la)
    # the same handle walks on: its second step is pass 42 at the parameters the first one left -- not c's (pass 42 at the initial ones)
    a.train_step(sup, qry)
    assert a.dropout_info() == dict(enabled=True, last_pass=42, next_pass=43, bytes=a.dropout_info()['bytes'])
    b.dropout_set_pass(42)
    b.train_step(sup, qry)
    same_state(state_of(a), state_of(b), 'set_pass')


# ----------------------------------------------------------------------------- (h) the MAML-style step's passes
def test_maml_style_step_advances_the_index_by_inner_steps_plus_one():
    cfg, sup, qry, B = case(3)
    model = new_model(cfg, max_sequences=B)
    model.dropout_enable(**DROP)
    for n, want in ((2, 3), (0, 4), (1, 6)):
        model.maml_step(sup, qry, n, 0.1)
        assert model.dropout_info()['next_pass'] == want
    model.maml_forward_backward(sup, qry, 3, 0.1)
    assert model.dropout_info()['next_pass'] == 10 and model.dropout_info()['last_pass'] == 9
    model.apply_update(1.0)
    model.maml_eval(sup, qry, 2, 0.1)
    assert model.dropout_info()['next_pass'] == 10


# ----------------------------------------------------------------------------- fp64, element by element
def drop_tensors(model, cfg, B, f):
    """the masked activations of every site the pass dropped, [B, T, W]; pads asserted to be exact zeros"""
    t = {}
    for site in range(cfg['n_layers'] + 1):
        if np.all(f[site] == 1):
            continue
        W = site_width(cfg, site)
        a = model.dropout_read(site, B)
        assert np.all(a[:, :, W:] == 0), 'pad columns of site %d' % site
        t[('drop', site)] = np.transpose(a[:, :, :W], (1, 0, 2))
    return t


def check_dropped(label, ref, got):
    """prints err / e32 of every tensor (the rows of tests/COMPONENTWISE_DROPOUT.md), holds the exact zeros, then asserts every bound"""
    failed = []
    for (fam, layer) in sorted(got, key=lambda k: (D.FAMILIES.index(k[0]), -1 if k[1] is None else k[1])):
        g = got[(fam, layer)]
        assert g.shape == ref.t[(fam, layer)].shape, (fam, layer, g.shape)
        if fam in ('drop', 'dx', 'dh'):
            zero = ref.zero_positions(fam, layer)
            print('DROPZ|%s|%s|%s|%d|%d|%d' % (label, fam, '' if layer is None else layer, int(zero.sum()), zero.size, int((g[zero] != 0).sum())))
            assert np.all(g[zero] == 0), '%s %s: nonzero at a dropped position' % (label, fam)
            if fam == 'drop':
                assert not np.signbit(g[zero]).any(), '%s: a dropped unit is +0.0' % label
        ratio, where = ref.ratio(fam, layer, g)
        bad = ref.failures(fam, layer, g, M)
        print('DROP|%s|%s|%s|%.2f|%.1e|%d|%s|%d/%d' % (label, fam, '' if layer is None else layer, ratio, ref.e32[fam], M,
                                                    tuple(int(i) for i in where), int(bad.sum()), bad.size))
        if bad.any():
            failed.append('%s%s: %d of %d outside M = %d (worst %.1f x e32 = %.1e at %s)'
                          % (fam, '' if layer is None else '_%d' % layer, int(bad.sum()), bad.size, M, ratio, ref.e32[fam], where))
    assert not failed, '%s: %s' % (label, '; '.join(failed))


def dropped_pass_against_fp64(label, cfg, sup, qry, B, drop, lengths=None, model=None, first_pass=7, fused=False, gemm_launches=None):
    """fused: dlogits stays in place, so the pass may take the fused softmax (asserted) and only the gradients and the masked
    activations are read; gemm_launches: the GEMM launches the pass must enqueue (fsmg_debug_read("gemm_kinds"))"""
    model = model or new_model(cfg, max_sequences=B)
    params = f64_params(model)
    model.dropout_enable(**drop)
    model.dropout_set_pass(first_pass)
    if not fused:
        model.debug_set('inplace_dlogits', 0)      # keep the logits beside dlogits
    kinds0 = model.debug_read('gemm_kinds', 4).copy()
    if lengths is None:
        X, Y = O.train_xy(sup, qry, cfg['input_size'])
        weights = None
        model.forward_backward(sup, qry)
    else:
        sl, ql = lengths
        X, Y = MR.device_xy(sup, qry, sl, ql, cfg)
        weights = MR.mask_of(MR.train_lengths(sl, ql), cfg['max_len'])
        model.forward_backward_masked(sup, qry, sl, ql)
    assert model.stats()['timeouts'] == 0
    if gemm_launches is not None:
        assert int((model.debug_read('gemm_kinds', 4) - kinds0).sum()) == gemm_launches
    if fused:
        assert list(model.debug_read('fused_softmax', 2)) == [1.0, 1.0]
    p = model.dropout_info()['last_pass']
    assert p == first_pass
    f = D.factors(cfg, drop, p, B)
    ref = D.DropReference(params, X, Y, cfg, f, weights)
    got = device_tensors(model, cfg, B, with_intermediates=not fused)
    got.update(drop_tensors(model, cfg, B, f))
    check_dropped(label, ref, got)
    return model, ref


@pytest.mark.parametrize('variational', [False, True], ids=['element', 'variational'])
@pytest.mark.parametrize('idx', IDX)
def test_every_tensor_of_a_dropped_pass_element_by_element(idx, variational, monkeypatch):
    monkeypatch.setenv('FSMG_GEMM', 'bx3')
    cfg, sup, qry, B = case(idx)
    drop = dict(DROP, variational=variational)
    model, ref = dropped_pass_against_fp64('%s|%s' % (R.shape_id(R.CW_SHAPES[idx]), 'var' if variational else 'elem'), cfg, sup, qry, B, drop)
    assert len([k for k in ref.t if k[0] == 'drop']) == cfg['n_layers'] + 1
    # the loss of the pass and tail[0] = sum of the MASKED dx^2 (the bound of tests/test_gpu_masked_componentwise.py)
    tail = model.debug_read('tail', 16)
    assert abs(float(tail[1]) - ref.loss) <= M * ref.e32['ce'] * ref.loss
    dx, S = ref.t[('dx', None)], ref.full['scales']['dx']
    tol = M * ref.e32['dx']
    want0 = ref.full['aux']['embedding_slices_sq']
    bound0 = 2 * tol * float((np.abs(dx) * S).sum()) + tol * tol * float((S * S).sum()) + 2.0 ** -24 * want0 + R.UNDERFLOW
    print('DROPL|%s|tail0 %.3f of its bound' % (R.shape_id(R.CW_SHAPES[idx]), abs(float(tail[0]) - want0) / bound0))
    assert abs(float(tail[0]) - want0) <= bound0


@pytest.mark.parametrize('which', ['keep_input', 'keep_output'])
@pytest.mark.parametrize('idx', [3, 5])
def test_one_keep_alone(idx, which, monkeypatch):
    monkeypatch.setenv('FSMG_GEMM', 'bx3')
    cfg, sup, qry, B = case(idx)
    drop = dict(keep_input=1.0, keep_output=1.0, variational=False, seed=SEED)
    drop[which] = 0.6
    model, ref = dropped_pass_against_fp64('%s|%s' % (R.shape_id(R.CW_SHAPES[idx]), which), cfg, sup, qry, B, drop)
    with pytest.raises(Exception, match='STATE'):          # the other kind of site launched nothing
        model.dropout_read(1 if which == 'keep_input' else 0, B)


# The readers of the masked copies that only wide shapes reach.  A pass enqueues 3 + 4 L GEMMs (projection, dH, dW; per layer zx, dKh, dKx,
# dx), one fewer for every layer whose dKx + dKh are ONE merged GEMM with a two-part A (api_backward.hip dk_merged_args; tests/test_gemm_forced.py
# counts the same way): the 256 x 256-tile kernel takes it where the layer's padded input width is a multiple of 256 and the rows suffice.
STACKED_WIDE = (dict(hidden_size=1024, embedding_size=16, input_size=60, max_len=20, n_layers=2), 5, 5, 4, 3)      # 900 rows >= 896


def test_fused_softmax_and_merged_dk_read_the_masked_copies_at_cfg_b_width(monkeypatch):
    """cfg-B at full width (45 x 46 rows), dlogits in place: the Hsc producer behind the fused softmax scales the MASKED top output, dW
    contracts it, and the merged dK of layer 0 reads the masked embedding rows without the gather (Ep = 256) -- gradients and drop<site>
    element by element, as tests/test_gpu_componentwise.py test_fused_softmax_gradients_element_by_element holds the undropped pass"""
    monkeypatch.setenv('FSMG_GEMM', 'bx3')
    over, N, K, Q, seed = FUSED
    cfg = small_config(**over)
    sup, qry = (a.astype(np.int32) for a in R.episode(cfg, N, K, Q, seed))
    B = N * (K + Q)
    model = new_model(cfg, max_sequences=B)
    assert model.debug_dims()['Ep'] % 256 == 0
    model, ref = dropped_pass_against_fp64('fused-%s' % R.shape_id(FUSED), cfg, sup, qry, B, DROP, model=model, fused=True, gemm_launches=3 + 4 - 1)
    assert {k for k in ref.t if k[0] == 'drop'} == {('drop', 0), ('drop', 1)}


def test_merged_dk_of_a_stacked_layer_reads_the_masked_output_below(monkeypatch):
    """hidden 1024 x 2 over 900 rows: layer 1's merged dK (in_p = Hp = 1024) reads drop_up(0); layer 0 (Ep = 16) keeps its two GEMMs"""
    monkeypatch.setenv('FSMG_GEMM', 'bx3')
    over, N, K, Q, seed = STACKED_WIDE
    cfg = small_config(**over)
    sup, qry = (a.astype(np.int32) for a in R.episode(cfg, N, K, Q, seed))
    B = N * (K + Q)
    assert B * cfg['max_len'] >= 896
    dropped_pass_against_fp64('wide-%s' % R.shape_id(STACKED_WIDE), cfg, sup, qry, B, DROP, gemm_launches=3 + 8 - 1)


@pytest.mark.parametrize('idx', [3, 5, 8])
def test_dropped_masked_pass_element_by_element(idx, monkeypatch):
    monkeypatch.setenv('FSMG_GEMM', 'bx3')
    cfg, sup, qry, B = case(idx)
    _, N, K, Q, seed = R.CW_SHAPES[idx]
    rng = np.random.RandomState(seed)
    sl, ql = MR.lengths_for(rng, (N, K), cfg['max_len']), MR.lengths_for(rng, (N, Q), cfg['max_len'])
    model, ref = dropped_pass_against_fp64('%s|masked' % R.shape_id(R.CW_SHAPES[idx]), cfg, sup, qry, B, DROP, lengths=(sl, ql))
    # the fused masked step at the same index: the same loss bits as the split form's pass
    other = new_model(cfg, max_sequences=B)
    other.dropout_enable(**DROP)
    other.dropout_set_pass(7)
    loss = other.train_step_masked(sup, qry, sl, ql)
    assert abs(loss - ref.loss) <= M * ref.e32['ce'] * ref.loss


def test_pass_repeated_after_a_time_out_draws_the_reported_masks(monkeypatch):
    """FSMG_CHAIN_SPIN_LIMIT=0 is the designed software time-out of tests/test_gpu_forced_componentwise.py.  The split form: the pass
    that timed out took index 7, the repeat is a new call and takes 8 -- held to fp64 with the masks of the index fsmg_dropout_info
    reports.  The fused step repeats INSIDE one call: it draws the masks of the pass it repeats and the counter moves by one."""
    from fsmg.binding import FsmgError
    env, over, N, K, Q, seed = R.FORCED_RECOVERY
    monkeypatch.setenv('FSMG_CHAIN_SPIN_LIMIT', '0')
    monkeypatch.setenv('FSMG_GEMM', 'bx3')
    cfg = small_config(**over)
    sup, qry = (a.astype(np.int32) for a in R.episode(cfg, N, K, Q, seed))
    B = N * (K + Q)
    model = new_model(cfg, max_sequences=B)
    params = f64_params(model)
    model.dropout_enable(**DROP)
    model.dropout_set_pass(7)
    model.debug_set('inplace_dlogits', 0)
    model.debug_set('fallback_steps', 2)
    model.forward_backward(sup, qry)
    with pytest.raises(FsmgError, match='persistent recurrent kernel timed out'):
        model.apply_update(1.0)
    assert model.stats()['timeouts'] == 1 and model.step == 0 and model.dropout_info()['last_pass'] == 7
    model.forward_backward(sup, qry)               # the repeat, on per-step launches
    p = model.dropout_info()['last_pass']
    assert p == 8
    f = D.factors(cfg, DROP, p, B)
    X, Y = O.train_xy(sup, qry, cfg['input_size'])
    ref = D.DropReference(params, X, Y, cfg, f)
    got = device_tensors(model, cfg, B)
    got.update(drop_tensors(model, cfg, B, f))
    check_dropped('forced-recovery|bx3', ref, got)
    # the fused step on a fresh handle: one time-out, one repeat inside the call, ONE index
    fused = new_model(cfg, max_sequences=B)
    fused.dropout_enable(**DROP)
    fused.dropout_set_pass(8)
    loss = fused.train_step(sup, qry)
    assert fused.stats()['timeouts'] == 1 and fused.step == 1
    assert fused.dropout_info()['last_pass'] == 8 and fused.dropout_info()['next_pass'] == 9
    assert abs(loss - ref.loss) <= M * ref.e32['ce'] * ref.loss


def test_three_maml_style_outer_steps_match_fp64():
    """losses to the project's 1e-4 relative, the parameters per tensor by rel_max < 5e-4 (tests/test_gpu_msgd.py's end-to-end bounds);
    every pass of the fp64 run takes numpy masks of the index the device's counter must have given it"""
    over, N, K, Q, seed = R.CW_SHAPES[3]
    cfg = small_config(**over)
    B = N * (K + Q)
    model = new_model(cfg, max_sequences=B)
    params = f64_params(model)
    opt = O.new_opt_state(params)
    model.dropout_enable(**DROP)
    n, lr = 2, 0.1
    eps = [tuple(a.astype(np.int32) for a in R.episode(cfg, N, K, Q, seed + s)) for s in range(3)]
    for s in range(3):
        want = D.maml_step_drop(params, opt, eps[s][0], eps[s][1], cfg, DROP, s * (n + 1), n, lr)
        got = model.maml_step(eps[s][0], eps[s][1], n, lr)
        print('DROP|maml|step %d|loss %.3e' % (s, abs(got - want) / abs(want)))
        assert abs(got - want) <= NLL_RTOL * abs(want), (s, got, want)
    assert model.dropout_info()['next_pass'] == 3 * (n + 1) and model.stats()['timeouts'] == 0 and model.step == 3
    for k in params:
        r = rel_max(model.get_param(k), params[k])
        print('DROP|maml|%s|theta %.2e' % (k, r))
        assert r < REL_MAX, (k, r)


# ----------------------------------------------------------------------------- refusals, plugin
def test_refusals_through_the_c_abi():
    cfg, sup, qry, B = case(1)
    m = new_model(cfg, max_sequences=B)
    with pytest.raises(Exception, match='STATE'):
        m.dropout_set_pass(3)
    nan = float('nan')
    for kw in (dict(keep_input=0.0), dict(keep_input=-0.5), dict(keep_input=1.5), dict(keep_input=nan), dict(keep_output=0.0),
               dict(keep_output=1.0001), dict(keep_output=nan), dict(variational=2)):
        with pytest.raises(Exception, match='INVALID'):
            m.dropout_enable(**kw)
    c = m.dropout_config(keep_input=0.5)
    c.struct_size = 8
    with pytest.raises(Exception, match='INVALID'):
        m.dropout_enable(c)
    info = m.dropout_info()
    assert not info['enabled'] and info['bytes'] == 0           # every refusal came before any device work
    m.dropout_enable(keep_input=0.5)
    assert m.dropout_info()['bytes'] > 0
    with pytest.raises(Exception, match='INVALID'):
        m.dropout_set_pass(-1)
    for args in ((-1, 0, B), (0, 2, B), (0, -1, B), (0, 0, 0)):
        with pytest.raises(Exception, match='INVALID'):
            m.dropout_mask(*args)
    with pytest.raises(Exception, match='STATE'):
        m.dropout_read(0, B)                                     # no dropped pass yet
    with pytest.raises(Exception, match='NAME'):
        m.debug_read('drop7', 4)


def test_plugin_on_the_golden_lyrics(tmp_path, golden_dir):
    import yaml
    from conftest import ROOT
    from data.episode import load_sampler_from_config
    from models.lstm_baseline import LSTMBaseline
    from test_masked_cpu import K, Q, T, _dataset, _raw_tree
    from test_train_entry import LOOP
    shipped = yaml.safe_load(open(os.path.join(ROOT, 'few-shot-music-generation_amd', 'src', 'config', 'lstm_dropout.yaml')))
    root = _raw_tree(tmp_path, golden_dir)
    _dataset(root)[0].metadata.close()
    full = dict(LOOP, name='lstm_dropout', model_module_name=shipped['model_module_name'], model_class_name=shipped['model_class_name'],
                n_decay=10000, lr=5e-3, max_grad_norm=5, embedding_size=32, hidden_size=40, n_layers=1, dataset='lyrics', dataset_path=root,
                splits=['train', 'val', 'test'], max_len=T, query_size=Q, support_size=K, seed=1234, split='train',
                keep_prob_input=shipped['keep_prob_input'], keep_prob_output=shipped['keep_prob_output'],
                dropout_variational=shipped['dropout_variational'], dropout_seed=9)
    sampler = load_sampler_from_config(dict(full))
    full['input_size'] = sampler.get_num_unique_words()
    eps = [sampler.get_episode() for _ in range(4)]
    plain = LSTMBaseline({k: v for k, v in full.items() if not (k.startswith('keep_prob') or k.startswith('dropout_'))})
    plain.recover_or_init('')
    assert plain.engine.dropout_info() == dict(enabled=False, last_pass=-1, next_pass=0, bytes=0)       # keys absent: never enabled
    model = LSTMBaseline(dict(full))
    model.recover_or_init('')
    assert model.engine.dropout_info()['enabled']
    assert np.float32(model.eval(eps[3])) == np.float32(plain.eval(eps[3]))                          # same seed, eval never drops
    losses = [model.train(e) for e in eps[:3]]
    plain_loss = plain.train(eps[0])
    assert all(np.isfinite(l) and l > 0 for l in losses) and losses[0] != plain_loss
    assert model.engine.dropout_info()['next_pass'] == 3
    nll = model.eval(eps[3])
    model.save(str(tmp_path / 'ck'))
    assert os.path.isfile(str(tmp_path / 'ck' / 'lstm_dropout' / 'lstm_dropout.dropout.npz'))
    again = LSTMBaseline(dict(full))
    again.recover_or_init(str(tmp_path / 'ck'))
    assert again.engine.dropout_info()['next_pass'] == 3 and again.engine.step == 3
    assert np.float32(again.eval(eps[3])) == np.float32(nll)
    assert np.float32(again.train(eps[3])) == np.float32(model.train(eps[3]))                         # the run continues with the same masks
