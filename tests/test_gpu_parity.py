"""-m gpu: the HIP path through the C-ABI vs the CPU oracle (fp64 restatement of the reference graph).

Bar (BASELINE.json north_star): NLL within 1e-4 relative of the CPU reference, fp32.  Intermediate
tensors and gradients are held to max|err| / max|ref| bounds written next to each check.
"""
import os

import numpy as np
import pytest

from conftest import free_port, small_config
from gpu_utils import f64_params, new_model, oracle_step, read_states, rel_max, time_major
from oracle import lstm_oracle as O

pytestmark = pytest.mark.gpu

NLL_RTOL = 1e-4

SHAPES = [
    # (config overrides, N, K, Q)
    (dict(), 2, 2, 1),                                                        # B=6: one partial M tile
    (dict(hidden_size=20, embedding_size=10, input_size=50, max_len=7), 1, 1, 1),   # H, E not multiples of 16/4
    (dict(hidden_size=48, embedding_size=24, input_size=301, max_len=9), 5, 5, 4),  # B=45 like cfg-B
    (dict(hidden_size=32, embedding_size=16, input_size=130, max_len=5), 10, 4, 3),  # B=70 > 48 rows: 2 row chunks
    (dict(hidden_size=32, embedding_size=12, input_size=77, max_len=6, n_layers=2), 3, 2, 2),   # stacked
    (dict(hidden_size=64, embedding_size=16, input_size=120, max_len=6), 3, 2, 2),                # Hp = 64: persistent chain kernels, 1 k-group per wave
    (dict(hidden_size=128, embedding_size=24, input_size=90, max_len=7), 5, 5, 4),               # Hp = 128, 3 row tiles: 2 k-groups per wave
    (dict(hidden_size=128, embedding_size=16, input_size=80, max_len=5), 20, 1, 4),               # 100 rows = 7 row tiles (cfg-D's episode shape) on the persistent kernels
    (dict(hidden_size=256, embedding_size=16, input_size=70, max_len=5), 4, 3, 2),                # Hp = 256: reduce-scatter BPTT kernel with 2 destination tiles per wave
    (dict(hidden_size=512, embedding_size=16, input_size=60, max_len=4), 2, 1, 1),                # Hp = 512 (cfg-B's recurrent shape): XCD-local kernels, 1 row group (4 rows on 4 XCDs)
    (dict(hidden_size=512, embedding_size=16, input_size=60, max_len=6), 5, 5, 4),                # ... 45 rows = 6 per XCD (3 on the last): 2 row groups, cfg-B's episode shape
    (dict(hidden_size=512, embedding_size=16, input_size=60, max_len=5), 20, 1, 4),               # ... 100 rows = 13 per XCD (9 on the last): 4 row groups, cfg-D's episode shape
    (dict(hidden_size=512, embedding_size=16, input_size=60, max_len=5, n_layers=2), 3, 3, 2),    # ... stacked: 15 rows = 2 per XCD (1 on the last)
    (dict(hidden_size=1024, embedding_size=16, input_size=60, max_len=4, n_layers=2), 2, 1, 1),   # Hp = 1024 (cfg-C's): 8 per wave, forward per step
    (dict(hidden_size=16, embedding_size=8, input_size=12500, max_len=4), 2, 1, 1),   # vocab rows > 12288 floats: 3-pass CE kernel
    (dict(hidden_size=16, embedding_size=8, input_size=7000, max_len=4), 2, 1, 1),    # 6144 < row <= 12288: 12-register CE kernel
    (dict(hidden_size=256, embedding_size=16, input_size=70, max_len=6), 5, 5, 4),    # Hp = 256: two row slices per XCD (k_lstm_*_slice), 45 rows = 3 per slice, 1 row group
    (dict(hidden_size=256, embedding_size=16, input_size=70, max_len=5), 20, 1, 4),   # ... 100 rows = 7 per slice: 2 row groups
    (dict(hidden_size=200, embedding_size=24, input_size=90, max_len=7), 5, 5, 4),    # the reference's default hidden size: padded to 256 inside, same kernels
    (dict(hidden_size=256, embedding_size=16, input_size=70, max_len=5, n_layers=2), 2, 2, 1),   # ... stacked, 6 rows on 6 slices
    (dict(hidden_size=320, embedding_size=250, input_size=300, max_len=6), 5, 5, 4),  # E = 250 pads to one 256-row tile: with FSMG_GEMM_H=2, dKx + dKh as ONE GEMM whose A is [gathered embedding rows | h_prev] and whose last row tile is partial
]


@pytest.fixture(params=['bx3', 'f32'])
def gemm_kind(request, monkeypatch):
    """both GEMM arithmetics of the library: the default bf16-split products on the bf16 matrix pipe and the fp32 MFMA
    (FSMG_GEMM=f32, the bench line's alt_gemm_f32_mfma leg) -- same tolerances for both"""
    monkeypatch.setenv('FSMG_GEMM', request.param)
    return request.param


_ORACLE_CACHE = {}


def cached_oracle_step(key, params, sup, qry, cfg):
    """the fp64 oracle of a full-size episode takes seconds: computed once per (test, shape), shared by the GEMM kinds
    (same seeded parameters, same episode)"""
    if key not in _ORACLE_CACHE:
        _ORACLE_CACHE[key] = oracle_step(params, sup, qry, cfg)
    return _ORACLE_CACHE[key]


def _episode(cfg, N, K, Q, seed=0, realistic=True):
    (sup, qry), = O.synthetic_episodes(1, N, K, Q, cfg['max_len'], cfg['input_size'], seed=seed, realistic=realistic)
    return sup, qry


@pytest.mark.parametrize('over,N,K,Q', SHAPES)
def test_forward_backward_every_tensor(over, N, K, Q, gemm_kind):
    cfg = small_config(**over)
    sup, qry = _episode(cfg, N, K, Q, seed=3)
    model = new_model(cfg, max_sequences=N * (K + Q))          # as the plugin does from the task YAML: picks the kernel family
    # hidden 512 with > 64 rows runs the bf16-split XCD-local recurrence (k_lstm_*_xcd16), every other shape the fp32 one
    forced = os.environ.get('FSMG_XCD_BX3')
    assert bool(model.debug_read('xcd_bx3', 1)[0]) == (cfg['hidden_size'] == 512 and (N * (K + Q) > 64 if forced is None else forced == '1'))
    params = f64_params(model)
    loss, cache, grads, aux = cached_oracle_step(('shape', repr(sorted(over.items())), N, K, Q), params, sup, qry, cfg)
    B, T = N * (K + Q), cfg['max_len']

    model.debug_set('inplace_dlogits', 0)      # keep the logits: by default the cross entropy writes dlogits over them
    model.forward_backward(sup, qry)
    tail = model.debug_read('tail', 16)
    assert abs(tail[1] - loss) <= NLL_RTOL * abs(loss)
    for l in range(cfg['n_layers']):
        hs, cs, _ = read_states(model, cfg, l, B)          # gates now hold dz (checked through the grads)
        assert rel_max(hs, cache['layers'][l]['hs']) < 2e-5, 'h layer %d' % l
        assert rel_max(cs, cache['layers'][l]['cs']) < 2e-5, 'c layer %d' % l
    V1p = model.debug_dims()['V1p']
    logits = model.debug_read('logits', B * T * V1p).reshape(B * T, V1p)[:, :cfg['input_size'] + 1]
    assert rel_max(logits, time_major(cache['logits'], B, T)) < 2e-5
    assert rel_max(model.debug_read('lse', B * T), time_major(cache['lse'], B, T)) < 1e-5
    assert rel_max(model.debug_read('ce', B * T), time_major(cache['ce'], B, T)) < 1e-5
    for name in grads:
        assert rel_max(model.get_grad(name), grads[name]) < 2e-4, name
    assert abs(tail[0] - aux['embedding_slices_sq']) <= 1e-4 * aux['embedding_slices_sq']


def test_embedding_gradient_of_tokens_that_occur_a_thousand_times():
    """Real episodes are zero padded behind each song's end and Zipf distributed: one token (the padding) holds a third of all positions,
    a handful of words dozens each.  Such a token's embedding gradient is summed in two levels (per 256-position chunk, then chunk by
    chunk: k_embed_grad_chunks) instead of by one block row after row (736 us of a 1.6 ms cfg-B step on such data), and the occurrence
    table is filled with one atomic per group of equal lanes.  2 880 positions in 12 chunks, about 1 100 of them token 0: every gradient
    against the fp64 oracle, twice on one handle (the owners must have put the table back) and bit for bit on a second handle."""
    cfg = small_config(hidden_size=64, embedding_size=40, input_size=500, max_len=96, n_layers=1)
    N, K, Q = 5, 3, 3
    sup, qry = _episode(cfg, N, K, Q, seed=17)
    counts = np.bincount(np.concatenate([sup.ravel(), qry.ravel()]), minlength=cfg['input_size'])
    assert counts[0] > 900 and (counts > 48).sum() >= 4, counts[:8]          # heavy tokens beside the padding
    model = new_model(cfg, max_sequences=N * (K + Q))
    params = f64_params(model)
    loss, cache, grads, aux = oracle_step(params, sup, qry, cfg)
    got = []
    for _ in range(2):
        model.forward_backward(sup, qry)
        tail = model.debug_read('tail', 16)
        assert abs(tail[1] - loss) <= NLL_RTOL * abs(loss)
        for name in grads:
            assert rel_max(model.get_grad(name), grads[name]) < 2e-4, name
        assert abs(tail[0] - aux['embedding_slices_sq']) <= 1e-4 * aux['embedding_slices_sq']
        got.append({k: model.get_grad(k).copy() for k in grads})
    other = new_model(cfg, max_sequences=N * (K + Q))
    other.forward_backward(sup, qry)
    for k in grads:
        np.testing.assert_array_equal(got[0][k], got[1][k])
        np.testing.assert_array_equal(got[0][k], other.get_grad(k))


@pytest.mark.parametrize('over,N,K,Q', [
    (dict(max_len=1), 2, 1, 1),                                         # a single time step: no recurrence at all
    (dict(max_len=2, input_size=1), 1, 1, 1),                           # a one-word vocabulary (V1 = 2 with the start word)
    (dict(embedding_size=1, hidden_size=1, input_size=5), 1, 1, 1),     # one unit, one embedding column
    (dict(hidden_size=512, embedding_size=8, input_size=30, max_len=3), 1, 0, 1),   # empty support set, one query song, XCD-local kernels with 1 row
    (dict(hidden_size=512, embedding_size=8, input_size=30, max_len=3), 16, 4, 4),  # 128 rows: the most the XCD-local kernels take
    (dict(hidden_size=512, embedding_size=8, input_size=30, max_len=3), 43, 2, 1),  # 129 rows: one more -> column-split / per-step kernels
])
def test_degenerate_and_boundary_shapes(over, N, K, Q):
    """Edge cases of the episode shape and the model dims (the reference feeds whatever the sampler yields: None batch dims,
    lstm_baseline.py:31-36): every gradient and one update against the oracle."""
    cfg = small_config(**over)
    rng = np.random.RandomState(5)
    sup = rng.randint(0, cfg['input_size'], size=(N, K, cfg['max_len'])).astype(np.int32)
    qry = rng.randint(0, cfg['input_size'], size=(N, Q, cfg['max_len'])).astype(np.int32)
    model = new_model(cfg)
    params = f64_params(model)
    loss, cache, grads, aux = oracle_step(params, sup, qry, cfg)
    model.forward_backward(sup, qry)
    assert abs(model.debug_read('tail', 16)[1] - loss) <= NLL_RTOL * abs(loss)
    for name in grads:
        assert rel_max(model.get_grad(name), grads[name]) < 2e-4, name
    opt = O.new_opt_state(params)
    O.apply_update(params, grads, aux, opt, cfg)
    assert abs(model.apply_update(1.0) - loss) <= NLL_RTOL * abs(loss)
    for name, ref in params.items():
        assert rel_max(model.get_param(name), ref) < 5e-4, name
    assert abs(model.eval_step(qry) - O.eval_step(params, qry, cfg)) <= NLL_RTOL * abs(loss)
    assert model.stats()['timeouts'] == 0


def test_forward_gates_before_backward():
    cfg = small_config()
    sup, qry = _episode(cfg, 2, 2, 1)
    model = new_model(cfg)
    params = f64_params(model)
    nll = model.eval_step(qry)
    X, Y = O.eval_xy(qry, cfg['input_size'])
    want, cache = O.forward(params, X, Y, cfg)
    assert abs(nll - want) <= NLL_RTOL * abs(want)
    _, _, gates = read_states(model, cfg, 0, X.shape[0])
    assert rel_max(gates, cache['layers'][0]['gates']) < 2e-5     # activated i, j, f(+1), o in reference gate order


@pytest.mark.parametrize('mode', ['tf1_slices', 'dense'])
@pytest.mark.parametrize('layers', [1, 2])
def test_ten_update_trajectory(mode, layers):
    """test_seed-style (reference src/train/test_seed.py): 10 consecutive train losses from identical
    parameters and episodes, plus the final weights and Adam state."""
    cfg = small_config(hidden_size=40, embedding_size=20, input_size=211, max_len=12, n_layers=layers,
                       max_grad_norm=0.3)      # small clip: the clip branch is active from step 0
    model = new_model(cfg, clip_norm_mode=mode)
    params = f64_params(model)
    opt = O.new_opt_state(params)
    for s in range(10):
        sup, qry = _episode(cfg, 3, 3, 2, seed=100 + s)
        want = O.train_step(params, opt, sup, qry, cfg, clip_norm_mode=mode)
        got = model.train_step(sup, qry)
        assert abs(got - want) <= NLL_RTOL * abs(want), (s, got, want)
    assert model.step == 10
    for name, ref in params.items():
        assert rel_max(model.get_param(name), ref) < 5e-4, name
        m, v = model.get_opt_state(name)
        assert rel_max(m, opt['m'][name]) < 2e-3, name
        assert rel_max(v, opt['v'][name]) < 4e-3, name
    np.testing.assert_allclose(model.read_losses(3)[-1], got, rtol=1e-6)


def test_sixty_update_trajectory_stays_inside_the_bar():
    """Error accumulation through Adam: 60 consecutive updates on learnable episodes (the loss falls
    5.7 -> ~2) stay within the NLL bar at every step.  Measured worst case 7.2e-6 (tools/trajectory_drift.py)."""
    cfg = small_config(hidden_size=48, embedding_size=24, input_size=301, max_len=16, n_layers=1)
    model = new_model(cfg)
    params = f64_params(model)
    opt = O.new_opt_state(params)
    episodes = O.synthetic_episodes(60, 3, 3, 2, cfg['max_len'], cfg['input_size'], seed=4, realistic=True)
    first = last = None
    for s, (sup, qry) in enumerate(episodes):
        want = O.train_step(params, opt, sup, qry, cfg)
        got = model.train_step(sup, qry)
        assert abs(got - want) <= 0.5 * NLL_RTOL * abs(want), (s, got, want)
        first = want if first is None else first
        last = want
    assert last < 0.6 * first          # the model actually learned; this is not parity on a flat loss


def test_clip_modes_differ_and_gnorm_matches():
    cfg = small_config(max_grad_norm=1e-3)
    sup, qry = _episode(cfg, 2, 2, 1)
    norms = {}
    for mode in ('tf1_slices', 'dense'):
        model = new_model(cfg, clip_norm_mode=mode)
        params = f64_params(model)
        _, _, grads, aux = oracle_step(params, sup, qry, cfg)
        model.train_step(sup, qry)
        norms[mode] = float(model.debug_read('gnorm', 1)[0])
        assert abs(norms[mode] - O.global_norm(grads, aux, mode)) <= 1e-4 * norms[mode]
    assert norms['tf1_slices'] != norms['dense']


def test_reference_default_dims_on_golden_episodes(golden_dir):
    """cfg-A: lyrics fixture episodes (captured from the reference sampler), E=250, H=200, T=32."""
    gold = np.load(os.path.join(golden_dir, 'g2_episodes.npz'))
    cfg = small_config(input_size=int(gold['vocab']), max_len=32, embedding_size=250, hidden_size=200)
    model = new_model(cfg)
    params = f64_params(model)
    opt = O.new_opt_state(params)
    for e in range(3):
        qry = gold['n2_val_%d_query' % e]
        want = O.eval_step(params, qry, cfg)
        assert abs(model.eval_step(qry) - want) <= NLL_RTOL * abs(want)
    for e in range(4):
        sup, qry = gold['n2_train_%d_support' % e], gold['n2_train_%d_query' % e]
        want = O.train_step(params, opt, sup, qry, cfg)
        got = model.train_step(sup, qry)
        assert abs(got - want) <= NLL_RTOL * abs(want), (e, got, want)


def test_eval_batch_equals_eval_steps_and_chunks():
    cfg = small_config(hidden_size=32, embedding_size=16, input_size=99, max_len=8)
    model = new_model(cfg, max_sequences=10)          # capacity 10 sequences -> 3 episodes of 3 per chunk
    eps = O.synthetic_episodes(7, 3, 2, 1, cfg['max_len'], cfg['input_size'], seed=5)
    queries = np.stack([q for _, q in eps])
    one_by_one = np.array([model.eval_step(q) for q in queries], np.float32)
    batched = model.eval_batch(queries)
    np.testing.assert_array_equal(batched, one_by_one)          # same kernels, rows independent -> bit-equal
    params = f64_params(model)
    for q, got in zip(queries, batched):
        want = O.eval_step(params, q, cfg)
        assert abs(got - want) <= NLL_RTOL * abs(want)


def test_eval_does_not_change_state_and_train_is_deterministic():
    cfg = small_config()
    sup, qry = _episode(cfg, 2, 2, 1)
    runs = []
    for _ in range(2):
        model = new_model(cfg)
        before = model.get_params()
        model.eval_step(qry)
        after = model.get_params()
        for k in before:
            np.testing.assert_array_equal(before[k], after[k])
        assert model.step == 0
        losses = [model.train_step(sup, qry) for _ in range(3)]
        runs.append((losses, model.get_params()))
    assert runs[0][0] == runs[1][0]
    for k in runs[0][1]:
        np.testing.assert_array_equal(runs[0][1][k], runs[1][1][k])     # no float atomics anywhere


def test_device_resident_tokens_match_host_tokens():
    import torch
    cfg = small_config()
    sup, qry = _episode(cfg, 2, 2, 1)
    a, b = new_model(cfg), new_model(cfg)
    ds, dq = torch.from_numpy(sup).cuda(), torch.from_numpy(qry).cuda()
    torch.cuda.synchronize()
    la = [a.train_step(sup, qry) for _ in range(2)]
    lb = [b.train_step(ds.data_ptr(), dq.data_ptr(), shape=(2, 2, 1)) for _ in range(2)]
    assert la == lb
    assert a.eval_step(qry) == b.eval_step(dq.data_ptr(), shape=(2, 1))


def test_indexed_step_on_a_device_resident_table_equals_the_token_step():
    """fsmg_upload_table + fsmg_train_step_indexed (the split's packed token table in HBM, an episode = row
    indices gathered on the GPU) gives the bits of fsmg_train_step on the gathered tokens; losses left in the device ring
    (want_loss=False) are the same numbers; a bad index is a token-range error and the update is skipped."""
    from fsmg.binding import FsmgError
    cfg = small_config(hidden_size=32, embedding_size=16, input_size=99, max_len=8)
    rng = np.random.RandomState(3)
    table = rng.randint(0, cfg['input_size'], size=(40, cfg['max_len'])).astype(np.int32)
    a, b = new_model(cfg), new_model(cfg)
    b.upload_table(0, table)
    want, got = [], []
    for s in range(4):
        si, qi = rng.randint(0, 40, size=(3, 2)), rng.randint(0, 40, size=(3, 2))
        want.append(a.train_step(table[si], table[qi]))
        got.append(b.train_step_indexed(0, si, qi, want_loss=(s % 2 == 0)))
    assert [g for g in got if g is not None] == want[0::2]
    np.testing.assert_array_equal(b.read_losses(4), np.array(want, np.float32))
    for k, v in a.get_params().items():
        np.testing.assert_array_equal(b.get_param(k), v)
    with pytest.raises(FsmgError, match='TOKEN_RANGE'):
        b.train_step_indexed(0, np.array([[40, 0]]), np.array([[1, 2]]))
    assert b.step == 4 and b.stats()['steps_skipped_token_range'] == 1
    with pytest.raises(FsmgError, match='STATE'):
        b.train_step_indexed(1, np.array([[0, 0]]), np.array([[1, 2]]))


def test_all_schedules_are_bit_identical(monkeypatch):
    """two-stream overlap (default, eager) == single stream replayed from hipGraphs == single stream eager"""
    cfg = small_config(hidden_size=32, embedding_size=16, input_size=99, max_len=8, n_layers=2)
    eps = O.synthetic_episodes(4, 3, 2, 2, cfg['max_len'], cfg['input_size'], seed=11)
    out = []
    for overlap, use_graph in (('1', True), ('0', True), ('0', False)):
        monkeypatch.setenv('FSMG_OVERLAP', overlap)
        model = new_model(cfg, use_graph=use_graph)
        losses = [model.train_step(s, q) for s, q in eps]            # graph mode: step 0 captures, 1.. replay
        evals = [model.eval_step(q) for _, q in eps]
        out.append((losses, evals, model.get_params()))
    for other in out[1:]:
        assert out[0][0] == other[0] and out[0][1] == other[1]
        for k in out[0][2]:
            np.testing.assert_array_equal(out[0][2][k], other[2][k])


def test_persistent_forward_chain_is_bit_identical(monkeypatch):
    """The column-split persistent kernels (one launch per chain chunk, h handed between blocks inside the launch; the default
    where they apply) compute exactly the bits of one launch per time step (FSMG_PERSISTENT=0), in both schedules."""
    cfg = small_config(hidden_size=128, embedding_size=32, input_size=150, max_len=24, n_layers=2)
    eps = O.synthetic_episodes(3, 5, 5, 4, cfg['max_len'], cfg['input_size'], seed=12)      # 45 rows: 3 row tiles
    out = []
    for persistent, overlap in (('0', '0'), ('1', '0'), ('1', '1')):
        monkeypatch.setenv('FSMG_PERSISTENT', persistent)
        monkeypatch.setenv('FSMG_OVERLAP', overlap)
        model = new_model(cfg)
        losses = [model.train_step(s, q) for s, q in eps]
        out.append((losses, model.get_params()))
    for other in out[1:]:
        assert out[0][0] == other[0]
        for k in out[0][1]:
            np.testing.assert_array_equal(out[0][1][k], other[1][k])


def test_all_row_tiles_forward_kernel_is_bit_identical(monkeypatch):
    """FSMG_FWD_RT=1 forces the persistent forward kernel that keeps a column tile for ALL row tiles in one block (what
    H = 1024 and 100-row episodes get by default): same bits as the one-row-tile kernel, 3 and 4 row tiles."""
    for (N, K, Q), hidden in (((5, 5, 4), 128), ((12, 1, 4), 64)):
        cfg = small_config(hidden_size=hidden, embedding_size=32, input_size=150, max_len=12, n_layers=2)
        eps = O.synthetic_episodes(2, N, K, Q, cfg['max_len'], cfg['input_size'], seed=16)
        out = []
        for rt in ('0', '1'):
            monkeypatch.setenv('FSMG_FWD_RT', rt)
            model = new_model(cfg)
            out.append(([model.train_step(s, q) for s, q in eps], model.get_params()))
        assert out[0][0] == out[1][0]
        for k in out[0][1]:
            np.testing.assert_array_equal(out[0][1][k], out[1][1][k])


def test_persistent_kernel_timeout_falls_back_and_repeats_the_step(monkeypatch):
    """FSMG_CHAIN_SPIN_LIMIT=0 makes every persistent kernel give up at its first wait (what happens when another
    workload keeps its blocks from becoming co-resident): the update is skipped on the device, the handle falls back to
    one launch per time step and fsmg_train_step repeats the step -- same numbers as a handle that never tried."""
    cfg = small_config(hidden_size=64, embedding_size=16, input_size=80, max_len=10)
    eps = O.synthetic_episodes(3, 3, 2, 2, cfg['max_len'], cfg['input_size'], seed=13)
    monkeypatch.setenv('FSMG_PERSISTENT', '0')
    ref = new_model(cfg)
    want = [ref.train_step(s, q) for s, q in eps]
    monkeypatch.setenv('FSMG_PERSISTENT', '1')
    monkeypatch.setenv('FSMG_CHAIN_SPIN_LIMIT', '0')
    model = new_model(cfg)
    got = [model.train_step(s, q) for s, q in eps]
    assert got == want and model.step == 3
    for k, v in ref.get_params().items():
        np.testing.assert_array_equal(model.get_param(k), v)
    # the split entry points report the failure instead of repeating (the caller owns the gradient exchange)
    model2 = new_model(cfg)
    model2.forward_backward(*eps[0])
    from fsmg.binding import FsmgError, RETRY_CODES
    with pytest.raises(FsmgError, match='persistent recurrent kernel timed out') as ei:
        model2.apply_update(1.0)
    assert ei.value.code == -9 and ei.value.code in RETRY_CODES and model2.step == 0      # FSMG_ERR_TIMEOUT: "skipped, repeat the call"
    model2.forward_backward(*eps[0])
    assert model2.apply_update(1.0) == want[0]


def test_inbox_refill_flag_survives_the_fallback_period():
    """a time-out leaves dh partials in the BPTT inboxes of the XCD-local kernels; the refill flag must stay
    up through the fallback steps (per-step kernels: no refill) until an XCD-local pass has really refilled.  Handle A times out
    on its second step (spin limit 0), repeats it and runs the next one on per-step launches, then goes back to the XCD-local
    kernels; handle B runs the same kernel families on the same episodes without ever timing out.  Same bits."""
    cfg = small_config(hidden_size=512, embedding_size=32, input_size=150, max_len=12)
    eps = O.synthetic_episodes(6, 5, 5, 4, cfg['max_len'], cfg['input_size'], seed=33)
    a, b = new_model(cfg), new_model(cfg)
    la, lb = [], []
    la.append(a.train_step(*eps[0])); lb.append(b.train_step(*eps[0]))
    assert a.stats()['xcd_launches'] > 0
    a.debug_set('fallback_steps', 3)
    a.debug_set('chain_spin_limit', 0)
    la.append(a.train_step(*eps[1]))                    # times out, is skipped on the device, repeated on per-step launches
    st = a.stats()
    assert st['timeouts'] == 1 and st['steps_skipped_timeout'] == 1 and not st['persistent_path'] and a.step == 2
    a.debug_set('chain_spin_limit', 1 << 18)
    b.debug_set('persistent', 0)
    lb.append(b.train_step(*eps[1]))
    la.append(a.train_step(*eps[2])); lb.append(b.train_step(*eps[2]))      # A: second fallback step
    b.debug_set('persistent', 1)
    x0 = a.stats()['xcd_launches']
    for e in eps[3:]:                                   # A: the persistent path is tried again -- on inboxes that still hold the aborted pass's partials
        la.append(a.train_step(*e)); lb.append(b.train_step(*e))
    st = a.stats()
    assert st['persistent_path'] and st['xcd_launches'] > x0 and st['timeouts'] == 1
    assert la == lb
    for k, v in b.get_params().items():
        np.testing.assert_array_equal(a.get_param(k), v)


def test_hidden_1024_recurrence_format_follows_the_train_passes(monkeypatch):
    """One handle (created for 45 sequences, two layers of 1024), train passes of 45, 20, 25, 45 and 45 rows: the pair kernels' format follows
    the row count -- bf16-split (k_lstm_*_pair16) from three row groups per weight copy on, fp32 row-group chains below (a MAML-style step
    is created for 45 sequences and runs passes of 25 and 20) -- with the weight images rewritten at every change.  Losses and parameters
    against a handle that stays on the fp32 pair kernels (FSMG_XCD_BX3=0): two arithmetics, both inside the parity bar."""
    cfg = small_config(hidden_size=1024, embedding_size=32, input_size=500, max_len=16, n_layers=2)
    shapes = [(5, 5, 4), (5, 2, 2), (5, 3, 2), (5, 5, 4), (5, 5, 4)]
    eps = [O.synthetic_episodes(1, n, k, q, cfg['max_len'], cfg['input_size'], seed=40 + i)[0] for i, (n, k, q) in enumerate(shapes)]
    a = new_model(cfg, max_sequences=45)
    monkeypatch.setenv('FSMG_XCD_BX3', '0')
    b = new_model(cfg, max_sequences=45)
    monkeypatch.delenv('FSMG_XCD_BX3')
    assert bool(a.debug_read('xcd_bx3', 1)[0]) and not bool(b.debug_read('xcd_bx3', 1)[0])
    seen = []
    for (n, k, q), ep in zip(shapes, eps):
        la, lb = a.train_step(*ep), b.train_step(*ep)
        assert abs(la - lb) <= NLL_RTOL * abs(lb), (n, k, q, la, lb)
        seen.append(bool(a.debug_read('xcd_bx3', 1)[0]))
        assert not bool(b.debug_read('xcd_bx3', 1)[0])
    assert seen == [True, False, False, True, True]
    for kname, v in b.get_params().items():
        assert rel_max(a.get_param(kname), v) < 5e-4, kname
    assert a.stats()['timeouts'] == 0


@pytest.mark.parametrize('order', ['serial', 'partitioned'])
def test_pair16_kernels_time_out_and_recover(order, monkeypatch):
    """Hidden 1024 on the bf16 matrix pipe (k_lstm_*_pair16, 45 rows, two stacked layers) under a forced time-out: the chain gives up at
    its first wait (spin limit 0: no probe, the sc1 poll fails at once), the step is skipped on the device and repeated on per-step
    launches, later steps go back to the pair kernels -- on BPTT inboxes that still hold the aborted pass's partials, which the
    same-XCD half of them received through the L2 (XCD_LOCAL_PLAIN) and the other half write-through.  Against a handle that runs the
    same kernel families without ever timing out: same bits.  `partitioned`: the opt-in XCD-partitioned order with every part on
    (packed chains, gated projection, dW and the queued dK beside the BPTT chains)."""
    if order == 'partitioned':
        monkeypatch.setenv('FSMG_XCD_OVERLAP', '1')
        monkeypatch.setenv('FSMG_XOV_PARTS', '7')
    cfg = small_config(hidden_size=1024, embedding_size=32, input_size=600, max_len=32, n_layers=2)
    eps = O.synthetic_episodes(5, 5, 5, 4, cfg['max_len'], cfg['input_size'], seed=36)
    a, b = new_model(cfg, max_sequences=45), new_model(cfg, max_sequences=45)
    assert bool(a.debug_read('xcd_bx3', 1)[0]) and (a.debug_read('xcd_partitioned', 2)[0] == 1.0) == (order == 'partitioned')
    la, lb = [a.train_step(*eps[0])], [b.train_step(*eps[0])]
    assert a.stats()['xcd_launches'] > 0
    a.debug_set('fallback_steps', 2)
    a.debug_set('chain_spin_limit', 0)
    la.append(a.train_step(*eps[1]))                    # times out, is skipped on the device, repeated on per-step launches
    st = a.stats()
    assert st['timeouts'] == 1 and st['steps_skipped_timeout'] == 1 and not st['persistent_path'] and a.step == 2
    a.debug_set('chain_spin_limit', 1 << 18)
    b.debug_set('persistent', 0)
    lb.append(b.train_step(*eps[1]))
    b.debug_set('persistent', 1)
    x0 = a.stats()['xcd_launches']
    for e in eps[2:]:
        la.append(a.train_step(*e)); lb.append(b.train_step(*e))
    st = a.stats()
    assert st['persistent_path'] and st['xcd_launches'] > x0 and st['timeouts'] == 1
    if order == 'serial':
        assert la == lb
        for k, v in b.get_params().items():
            np.testing.assert_array_equal(a.get_param(k), v)
    else:                                               # (the fallback step of A ran the serial order's K splits: close, not the same bits)
        assert np.allclose(la, lb, rtol=1e-5)
        for k, v in b.get_params().items():
            assert rel_max(a.get_param(k), v) < 1e-4, k


def test_partitioned_schedule_times_out_and_recovers(monkeypatch):
    """The XCD-partitioned order under a forced time-out: the packed chain gives up at its first wait (spin limit 0), the gated
    projection tiles see the flag and leave, the step is skipped on the device and repeated on per-step launches; later steps go
    back to the partitioned order.  Against a handle that runs the same kernel families without ever timing out: same bits."""
    monkeypatch.setenv('FSMG_XCD_OVERLAP', '1')
    cfg = small_config(hidden_size=512, embedding_size=32, input_size=3000, max_len=32)
    eps = O.synthetic_episodes(5, 5, 5, 4, cfg['max_len'], cfg['input_size'], seed=35)
    a, b = new_model(cfg, max_sequences=45), new_model(cfg, max_sequences=45)
    assert a.debug_read('xcd_partitioned', 2)[0] == 1.0 and bool(a.debug_read('xcd_bx3', 1)[0])
    la, lb = [a.train_step(*eps[0])], [b.train_step(*eps[0])]
    a.debug_set('fallback_steps', 2)
    a.debug_set('chain_spin_limit', 0)
    la.append(a.train_step(*eps[1]))
    st = a.stats()
    assert st['timeouts'] == 1 and st['steps_skipped_timeout'] == 1 and a.step == 2
    a.debug_set('chain_spin_limit', 1 << 18)
    b.debug_set('persistent', 0)
    lb.append(b.train_step(*eps[1]))
    b.debug_set('persistent', 1)
    for e in eps[2:]:
        la.append(a.train_step(*e)); lb.append(b.train_step(*e))
    assert a.stats()['persistent_path'] and a.stats()['timeouts'] == 1
    assert la == lb
    for k, v in b.get_params().items():
        np.testing.assert_array_equal(a.get_param(k), v)


def test_eager_and_graph_replayed_passes_give_the_same_bits():
    """Passes on the persistent recurrent kernels are issued eagerly by default (the caller's device token buffers are read in
    place); debug_set('eager', 0) replays them from hipGraphs with staged tokens.  Same kernels, same order: same bits."""
    import torch
    cfg = small_config(hidden_size=512, embedding_size=32, input_size=150, max_len=12)
    eps = O.synthetic_episodes(4, 5, 5, 4, cfg['max_len'], cfg['input_size'], seed=34)
    a, b = new_model(cfg), new_model(cfg)
    b.debug_set('eager', 0)
    dev = [(torch.from_numpy(s_).cuda(), torch.from_numpy(q_).cuda()) for s_, q_ in eps]
    la = [a.train_step(ds.data_ptr(), dq.data_ptr(), shape=(5, 5, 4)) for ds, dq in dev]
    lb = [b.train_step(ds.data_ptr(), dq.data_ptr(), shape=(5, 5, 4)) for ds, dq in dev]
    lc = [new_model(cfg).train_step(*eps[0])]                                  # host tokens through the staging buffer
    assert la == lb and lc[0] == la[0]
    for k, v in b.get_params().items():
        np.testing.assert_array_equal(a.get_param(k), v)


def test_xcd_local_and_column_split_kernels_agree_and_fall_back(monkeypatch):
    """Hidden size 512 takes the XCD-local recurrence (csrc/lstm_xcd.hip) by default.  FSMG_XCD=0 keeps the column-split
    persistent kernels: a different summation order (K split 4 x 128 per wave in both, but 16-wide k groups in another
    order), so not the same bits -- both within the bar of the oracle and 1e-5 of each other after three updates.  A forced
    time-out (FSMG_CHAIN_SPIN_LIMIT=0) makes the handle repeat the step with one launch per time step."""
    cfg = small_config(hidden_size=512, embedding_size=32, input_size=150, max_len=12)
    eps = O.synthetic_episodes(3, 5, 5, 4, cfg['max_len'], cfg['input_size'], seed=31)
    out = {}
    for xcd in ('1', '0'):
        monkeypatch.setenv('FSMG_XCD', xcd)
        model = new_model(cfg)
        params = f64_params(model)
        opt = O.new_opt_state(params)
        losses = []
        for s_, q_ in eps:
            want = O.train_step(params, opt, s_, q_, cfg)
            got = model.train_step(s_, q_)
            assert abs(got - want) <= NLL_RTOL * abs(want)
            losses.append(got)
        stats = model.stats()
        assert (stats['xcd_launches'] > 0) == (xcd == '1') and stats['timeouts'] == 0
        out[xcd] = (losses, model.get_params())
    for a, b in zip(out['1'][0], out['0'][0]):
        assert abs(a - b) <= 1e-5 * abs(b)
    monkeypatch.setenv('FSMG_XCD', '1')
    monkeypatch.setenv('FSMG_CHAIN_SPIN_LIMIT', '0')
    model = new_model(cfg)
    got = [model.train_step(s_, q_) for s_, q_ in eps]
    assert model.step == 3 and model.stats()['timeouts'] == 1
    for a, b in zip(got, out['1'][0]):
        assert abs(a - b) <= 1e-5 * abs(b)


def test_training_keeps_the_persistent_path_after_a_large_validation_batch():
    """A validation batch grows the activation scratch to hundreds of rows; the hand-off buffers of the persistent BPTT
    kernel must survive that (they are sized per hidden size, not per batch) -- observable through the forced-timeout
    knob: only a persistent launch can time out."""
    cfg = small_config(hidden_size=128, embedding_size=16, input_size=60, max_len=6)
    eps = O.synthetic_episodes(2, 3, 2, 2, cfg['max_len'], cfg['input_size'], seed=14)
    model = new_model(cfg)
    big = np.stack([q for _, q in O.synthetic_episodes(16, 10, 1, 4, cfg['max_len'], cfg['input_size'], seed=15)])   # 640 rows
    model.eval_batch(big)
    os.environ['FSMG_CHAIN_SPIN_LIMIT'] = '0'          # read at create time: does not touch `model`
    try:
        probe = new_model(cfg)
        probe.eval_batch(big)
        probe.forward_backward(*eps[0])
        with pytest.raises(Exception, match='persistent recurrent kernel timed out'):
            probe.apply_update(1.0)
    finally:
        del os.environ['FSMG_CHAIN_SPIN_LIMIT']
    assert np.isfinite(model.train_step(*eps[0]))


def test_split_k_paths_match_oracle_at_wide_shapes():
    """rows = 45*40 = 1800 with H=128: the dK / dH / dW GEMMs take the split-K + slab-reduce path."""
    cfg = small_config(hidden_size=128, embedding_size=64, input_size=1500, max_len=40)
    (sup, qry), = O.synthetic_episodes(1, 5, 5, 4, cfg['max_len'], cfg['input_size'], seed=2, realistic=True)
    model = new_model(cfg)
    params = f64_params(model)
    loss, cache, grads, aux = oracle_step(params, sup, qry, cfg)
    model.forward_backward(sup, qry)
    assert abs(model.debug_read('tail', 16)[1] - loss) <= NLL_RTOL * abs(loss)
    for name in grads:
        assert rel_max(model.get_grad(name), grads[name]) < 2e-4, name


def test_split_step_equals_fused_step():
    cfg = small_config()
    sup, qry = _episode(cfg, 2, 2, 1)
    a, b = new_model(cfg), new_model(cfg)
    la = a.train_step(sup, qry)
    b.forward_backward(sup, qry)
    lb = b.apply_update(1.0)
    assert la == lb
    for k, v in a.get_params().items():
        np.testing.assert_array_equal(v, b.get_param(k))


def test_errors():
    from fsmg.binding import FsmgError
    cfg = small_config()
    model = new_model(cfg)
    sup, qry = _episode(cfg, 2, 2, 1)
    bad = qry.copy()
    bad[0, 0, 3] = cfg['input_size']            # the start word is not a legal data token
    with pytest.raises(FsmgError, match='TOKEN_RANGE'):
        model.eval_step(bad)
    assert np.isfinite(model.eval_step(qry))    # the handle stays usable
    with pytest.raises(FsmgError, match='STATE'):
        model.apply_update(1.0)
    with pytest.raises(FsmgError, match='NAME'):
        model.get_param('nope')
    with pytest.raises(ValueError):
        model.eval_step(qry[:, :, :-1])
    with pytest.raises(FsmgError, match='INVALID'):
        new_model(small_config(hidden_size=0))


def test_param_roundtrip_and_opt_state_roundtrip():
    cfg = small_config(hidden_size=20, embedding_size=10, n_layers=2)
    model = new_model(cfg)
    ref = O.glorot_init(cfg, 9, np.float32)
    model.set_params(ref)
    for k, v in ref.items():
        np.testing.assert_array_equal(model.get_param(k), v)
        model.set_opt_state(k, v * 2, v * v)
        m, vv = model.get_opt_state(k)
        np.testing.assert_array_equal(m, v * 2)
        np.testing.assert_array_equal(vv, v * v)
    model.step = 77
    assert model.step == 77


def test_init_distribution_is_glorot_uniform():
    cfg = small_config(hidden_size=64, embedding_size=32, input_size=499)
    model = new_model(cfg)
    p = model.get_params()
    for name, w in p.items():
        if name.startswith('bias_'):
            assert np.all(w == 0)
            continue
        fan_in, fan_out = (w.shape[0], w.shape[0]) if w.ndim == 1 else w.shape
        limit = np.sqrt(6.0 / (fan_in + fan_out))
        assert np.abs(w).max() <= limit and np.abs(w).max() > 0.9 * limit, name
        assert abs(w.mean()) < 0.05 * limit and abs(w.std() - limit / np.sqrt(3)) < 0.05 * limit, name


def test_sample_matches_oracle_greedy_decode():
    cfg = small_config(hidden_size=24, embedding_size=12, input_size=61, n_layers=2)
    model = new_model(cfg)
    sup, qry = _episode(cfg, 2, 2, 1)
    for _ in range(3):
        model.train_step(sup, qry)
    params = f64_params(model)
    assert model.sample(15) == O.sample(params, 15, cfg)


@pytest.mark.parametrize('layers,inner_steps,hidden', [(1, 1, 40), (2, 2, 40), (1, 1, 512)])
def test_maml_step_and_eval_match_oracle(layers, inner_steps, hidden):
    """cfg-E (BASELINE.json configs[4]): three outer steps of the first-order MAML-style loop -- per episode `inner_steps`
    clipped SGD steps on the support rows, query loss and gradient at the adapted parameters, clip + Adam on theta -- and
    the few-shot evaluation, against oracle/lstm_oracle.py maml_step / maml_eval (itself checked against torch autograd).
    hidden 512 takes the XCD-local recurrent kernels (support 15 rows, query 10 rows)."""
    cfg = small_config(hidden_size=hidden, embedding_size=20, input_size=211, max_len=12, n_layers=layers, max_grad_norm=0.5)
    inner_lr = 0.3
    model = new_model(cfg)
    params = f64_params(model)
    opt = O.new_opt_state(params)
    eps = O.synthetic_episodes(4, 5, 3, 2, cfg['max_len'], cfg['input_size'], seed=41, realistic=True)
    want_eval = O.maml_eval(params, eps[3][0], eps[3][1], cfg, inner_steps, inner_lr)
    got_eval = model.maml_eval(eps[3][0], eps[3][1], inner_steps, inner_lr)
    assert abs(got_eval - want_eval) <= NLL_RTOL * abs(want_eval)
    plain = O.eval_step(params, eps[3][1], cfg)
    assert abs(want_eval - plain) > 10 * NLL_RTOL * abs(plain)          # the adaptation moves the NLL: the check has teeth
    for name, ref in params.items():                                    # evaluation left theta alone
        assert rel_max(model.get_param(name), ref) == 0.0, name
    for s, (sup, qry) in enumerate(eps[:3]):
        want = O.maml_step(params, opt, sup, qry, cfg, inner_steps, inner_lr)
        got = model.maml_step(sup, qry, inner_steps, inner_lr)
        assert abs(got - want) <= NLL_RTOL * abs(want), (s, got, want)
    assert model.step == 3
    for name, ref in params.items():
        assert rel_max(model.get_param(name), ref) < 5e-4, name
    # split form (what an episode-parallel rank runs): gradients in the buffer, theta untouched until apply_update
    before = model.get_params()
    model.maml_forward_backward(eps[3][0], eps[3][1], inner_steps, inner_lr)
    _, grads, aux = O.maml_query_grads(params, eps[3][0], eps[3][1], cfg, inner_steps, inner_lr)
    for name in grads:
        assert rel_max(model.get_grad(name), grads[name]) < 5e-4, name
        np.testing.assert_array_equal(model.get_param(name), before[name])


def test_maml_plugin_runs_through_the_models_api(tmp_path):
    from data.episode import Episode
    from models.maml_lstm import MAMLLSTM
    cfg = small_config(name='maml_lstm', inner_steps=2, inner_lr=0.2, checkpt_dir=str(tmp_path))
    sup, qry = _episode(cfg, 3, 3, 2)
    ep = Episode(sup, qry)
    m = MAMLLSTM(dict(cfg))
    m.recover_or_init('')
    params = {k: v.astype(np.float64) for k, v in m.engine.get_params().items()}
    opt = O.new_opt_state(params)
    assert abs(m.eval(ep) - O.maml_eval(params, sup, qry, cfg, 2, 0.2)) <= NLL_RTOL * 10
    for _ in range(2):
        want = O.maml_step(params, opt, sup, qry, cfg, 2, 0.2)
        assert abs(m.train(ep) - want) <= NLL_RTOL * abs(want)
    assert m.eval_many([ep, ep]) == [m.eval(ep)] * 2 and len(m.sample(sup[0], 4)) == 4


def test_plugin_api_checkpoint_resume(tmp_path):
    from data.episode import Episode
    from models.lstm_baseline import LSTMBaseline
    cfg = small_config(checkpt_dir=str(tmp_path))
    sup, qry = _episode(cfg, 2, 2, 1)
    ep = Episode(sup, qry)
    a = LSTMBaseline(dict(cfg))
    assert a.name == 'lstm_baseline'
    with pytest.raises(RuntimeError):
        a.train(ep)                              # recover_or_init first
    a.recover_or_init('')
    l1 = [a.train(ep) for _ in range(3)]
    a.save(str(tmp_path))
    l2 = [a.train(ep) for _ in range(2)]
    b = LSTMBaseline(dict(cfg))
    b.recover_or_init(str(tmp_path))             # weights + Adam slots + global_step come back
    assert b.engine.step == 3
    assert [b.train(ep) for _ in range(2)] == l2
    assert b.eval(ep) == a.eval(ep)
    assert a.eval_many([ep, ep]) == [a.eval(ep)] * 2
    assert os.path.isfile(os.path.join(str(tmp_path), 'lstm_baseline', 'lstm_baseline-3.npz'))
    assert len(a.sample(sup[0], 5)) == 5 and l1[0] > 0


# ------------------------------------------------------------------ full-size configurations (BASELINE.json configs)
FULL = {
    'cfg-B': (dict(input_size=10000, max_len=128, embedding_size=250, hidden_size=512, n_layers=1), 5, 5, 4),
    'cfg-C': (dict(input_size=4708, max_len=50, embedding_size=250, hidden_size=1024, n_layers=2), 5, 5, 4),
    'cfg-D': (dict(input_size=10000, max_len=128, embedding_size=250, hidden_size=512, n_layers=1), 20, 1, 4),
    # "cfg-C: ... T = 50 (YAML) and 128" -- the two layers of 1024 at the headline's sequence length (637 GFLOP per episode)
    'cfg-C-T128': (dict(input_size=4708, max_len=128, embedding_size=250, hidden_size=1024, n_layers=2), 5, 5, 4),
}
# BASELINE.json configs[4]: the MAML-style loop at its own size (freemidi vocabulary, 2-layer LSTM h=1024, 5-way / 5-shot);
# it has its own test (a baseline step at these dims IS cfg-C)
FULL_E = (dict(input_size=4708, max_len=50, embedding_size=250, hidden_size=1024, n_layers=2), 5, 5, 4, 1, 0.1)


@pytest.mark.parametrize('name', sorted(FULL))
def test_full_size_properties(name):
    """At BASELINE.json's full sizes the fp64 oracle is too slow for a trajectory, so check size-independent
    properties: untrained NLL ~ ln(V1); eval of the query set == the same rows inside eval_batch; training on
    one episode repeatedly lowers its loss monotonically at first; loss is finite and run-to-run bit-stable;
    and ONE oracle eval (forward only, fp64) pins the full-size forward to 1e-4."""
    over, N, K, Q = FULL[name]
    cfg = small_config(**over)
    (sup, qry), (sup2, qry2) = O.synthetic_episodes(2, N, K, Q, cfg['max_len'], cfg['input_size'], seed=21)
    model = new_model(cfg, max_sequences=N * (K + Q))
    nll0 = model.eval_step(qry)
    assert abs(nll0 - np.log(cfg['input_size'] + 1)) < 0.02
    want = O.eval_step(f64_params(model), qry, cfg)
    assert abs(nll0 - want) <= NLL_RTOL * abs(want)
    both = model.eval_batch(np.stack([qry, qry2]))
    assert both[0] == np.float32(nll0) and both[1] == np.float32(model.eval_step(qry2))
    losses = [model.train_step(sup, qry) for _ in range(4)]
    assert np.all(np.isfinite(losses)) and losses[0] > losses[1] > losses[2]
    # (the fourth update overshoots at cfg-C's T = 128 -- two layers of 1024 at lr 5e-3 on one repeated episode: 8.457, 8.447, 8.170, 8.844;
    # the gradients and the update of that size are pinned against the fp64 oracle in test_full_size_gradients_match_oracle)
    assert losses[2] > losses[3] or name == 'cfg-C-T128'
    again = new_model(cfg)
    assert [again.train_step(sup, qry) for _ in range(4)] == losses


def test_graph_replay_equals_eager_launches_at_full_size(monkeypatch):
    """cfg-B runs single-stream from a hipGraph (captured at the first step, replayed afterwards).  Three steps on
    different episodes -- i.e. one capture and two REPLAYS -- must give the bits of the same launches issued eagerly.  (A
    replayed graph holding hipMemsetAsync nodes left garbage in the zero-state block of the hidden states from the second
    launch on; the step now fills with a kernel.  Found by the fresh-handle screen below.)"""
    over, N, K, Q = FULL['cfg-B']
    cfg = small_config(**over)
    eps = O.synthetic_episodes(3, N, K, Q, cfg['max_len'], cfg['input_size'], seed=23)
    out = []
    for graph in ('1', '0'):
        monkeypatch.setenv('FSMG_GRAPH', graph)
        model = new_model(cfg)
        losses = [model.train_step(s_, q_) for s_, q_ in eps]
        model.forward_backward(*eps[0])
        grads = {k: model.get_grad(k) for k in model.param_shapes}
        out.append((losses, grads, model.get_params()))
        assert all(np.isfinite(v).all() and np.abs(v).max() < 1.0 for v in grads.values())
    assert out[0][0] == out[1][0]
    for k in out[0][1]:
        np.testing.assert_array_equal(out[0][1][k], out[1][1][k])
        np.testing.assert_array_equal(out[0][2][k], out[1][2][k])


def test_bf16_split_gemm_is_no_less_accurate_than_the_fp32_mfma_gemm(monkeypatch):
    """The default GEMM (k_gemm_bx3, csrc/gemm.hip) assembles every fp32 product from bf16 pieces on the bf16 matrix pipe:
    a = a1 + a2 + a3 exactly, six partial products, fp32 accumulation.  The claim that makes this an fp32 computation and
    not a reduced-precision one: against the fp64 oracle it is at least as close as the fp32-MFMA GEMM (FSMG_GEMM=f32) on
    the loss, the logits' statistics and every gradient tensor (RMS error; 1.5x slack for tensors whose error is dominated
    by the shared fp32 recurrence), at a shape that takes the production kernels (hidden 512, split-K weight gradients)."""
    cfg = small_config(hidden_size=512, embedding_size=250, input_size=3000, max_len=48)
    N, K, Q = 5, 5, 4
    (sup, qry), = O.synthetic_episodes(1, N, K, Q, cfg['max_len'], cfg['input_size'], seed=31, realistic=True)
    err = {}
    for kind in ('f32', 'bx3'):
        monkeypatch.setenv('FSMG_GEMM', kind)
        model = new_model(cfg)
        if kind == 'f32':
            params = f64_params(model)
            loss, cache, grads, aux = oracle_step(params, sup, qry, cfg)
        model.forward_backward(sup, qry)
        tail = model.debug_read('tail', 16)
        e = {'loss': abs(tail[1] - loss) / abs(loss)}
        for name in grads:
            d = model.get_grad(name).astype(np.float64) - grads[name]
            e[name] = float(np.sqrt(np.mean(d * d)) / np.sqrt(np.mean(grads[name] ** 2)))
        err[kind] = e
    for name in err['f32']:
        assert err['bx3'][name] <= 1.5 * err['f32'][name] + 1e-7, (name, err['bx3'][name], err['f32'][name])
    assert err['bx3']['loss'] <= NLL_RTOL
    assert max(v for k, v in err['bx3'].items() if k != 'loss') < 2e-5


def test_xcd_partitioned_schedule_gives_the_same_bits(monkeypatch):
    """FSMG_XCD_OVERLAP=1 (fsmg_config.schedule = XCD_PARTITIONED): the bf16-split recurrence packs the 45
    rows on three XCDs and publishes the time steps it has finished; the projection's 256 x 256 tiles are drawn from a work queue
    by the other five XCDs as their rows arrive (and by the whole chip once the chain is over); backward, dW's tiles run beside
    the BPTT chain the same way.  Which XCD computes a tile, and when, must not change a bit: against the SAME kernels in the
    serial order (FSMG_XCD_BX3=1) the forward pair alone gives identical losses and gradients; with the backward pair only dW / dd
    change their summation order (K split 6 instead of 3)."""
    over, N, K, Q = FULL['cfg-B']
    cfg = small_config(**over)
    eps = O.synthetic_episodes(3, N, K, Q, cfg['max_len'], cfg['input_size'], seed=29)
    out = []
    monkeypatch.setenv('FSMG_XCD_BX3', '1')
    for xov, parts in (('0', '3'), ('1', '1'), ('1', '3')):
        monkeypatch.setenv('FSMG_XCD_OVERLAP', xov)
        monkeypatch.setenv('FSMG_XOV_PARTS', parts)
        model = new_model(cfg)
        losses = [model.train_step(s_, q_) for s_, q_ in eps]
        model.forward_backward(*eps[0])
        out.append((losses, {k: model.get_grad(k) for k in model.param_shapes}, model.stats()))
    assert out[0][0] == out[1][0]
    for k in out[0][1]:
        np.testing.assert_array_equal(out[0][1][k], out[1][1][k])
        # (three updates with a dW that differs in its last bits: every tensor of the fourth pass may differ in ITS last bits)
        np.testing.assert_allclose(out[2][1][k], out[0][1][k], rtol=0, atol=1e-5 * np.abs(out[0][1][k]).max())
    np.testing.assert_allclose(out[2][0], out[0][0], rtol=1e-6)
    assert all(st['timeouts'] == 0 and st['xcd_launches'] > 0 for _, _, st in out)


def test_partitioned_order_with_episode_shapes_that_change_from_call_to_call(monkeypatch):
    """The plugin contract lets N, K, Q differ from call to call (the reference's placeholders have a free batch dimension).  One
    handle created for cfg-B's 45 sequences then sees 45, 18, 30, 6, 60 (more than it was sized for: buffers grow), 45 rows: calls whose
    row count the packed chains take run the XCD-partitioned order, the others fall to the serial one -- same losses as a handle that
    never leaves the serial order (the forward is bit-identical per call; dW's K split differs, so later losses agree to rounding),
    no time-out, no stale queue words or progress counters from a call of another shape."""
    over, N, K, Q = FULL['cfg-B']
    cfg = small_config(**dict(over, max_len=48))
    shapes = [(5, 5, 4), (2, 5, 4), (5, 3, 3), (3, 1, 1), (6, 5, 5), (5, 5, 4), (2, 5, 4), (5, 5, 4)]
    eps = [O.synthetic_episodes(1, n, k, q, cfg['max_len'], cfg['input_size'], seed=40 + i)[0] for i, (n, k, q) in enumerate(shapes)]
    runs = {}
    for xov in ('0', '1'):
        monkeypatch.setenv('FSMG_XCD_OVERLAP', xov)
        model = new_model(cfg, max_sequences=45)
        losses, used = [], []
        for s_, q_ in eps:
            losses.append(model.train_step(s_, q_))
            used.append(int(model.debug_read('xcd_partitioned', 3)[2]))
        runs[xov] = (losses, used, model.stats(), {k: model.get_param(k) for k in model.param_shapes})
        model.close()
    assert all(np.isfinite(runs['1'][0])) and runs['1'][2]['timeouts'] == 0 and runs['0'][2]['timeouts'] == 0
    assert not any(runs['0'][1]) and runs['1'][1][0] == 1 and runs['1'][1][5] == 1, runs['1'][1]      # 45 rows: partitioned; the serial handle never
    assert runs['1'][0][0] == runs['0'][0][0]                                                          # first call: same bits
    np.testing.assert_allclose(runs['1'][0], runs['0'][0], rtol=2e-6)
    for k in runs['0'][3]:
        # (Adam's m / sqrt(v) amplifies last-bit gradient differences on rarely touched embedding rows: a few elements move by 1e-4 of the largest)
        np.testing.assert_allclose(runs['1'][3][k], runs['0'][3][k], rtol=0, atol=1e-3 * max(np.abs(runs['0'][3][k]).max(), 1e-3))


def test_fresh_handles_reproduce_each_other_bit_for_bit_at_cfg_b():
    """Race screen (tools/race_hunt2.py in small): 100 fresh handles, two train steps each on DIFFERENT episodes (so a
    stale buffer of the previous handle or step would carry different data), every gradient and parameter identical
    to the first handle's.  This is the test that exposed the LDS write-after-read race of the persistent forward
    kernel (about one pass in 300, two-stream schedule only)."""
    over, N, K, Q = FULL['cfg-B']
    cfg = small_config(**over)
    eps = O.synthetic_episodes(2, N, K, Q, cfg['max_len'], cfg['input_size'], seed=22)
    ref = None
    for rep in range(100):
        model = new_model(cfg)
        model.forward_backward(*eps[0])
        g1 = {k: model.get_grad(k).tobytes() for k in model.param_shapes}
        model.apply_update(1.0)
        loss2 = model.train_step(*eps[1])
        cur = (g1, loss2, {k: v.tobytes() for k, v in model.get_params().items()})
        if ref is None:
            ref = cur
        else:
            assert cur[1] == ref[1], rep
            assert all(cur[0][k] == ref[0][k] for k in ref[0]), rep
            assert all(cur[2][k] == ref[2][k] for k in ref[2]), rep
        model.close()


def test_nccl_allreduce_runs_on_the_gradient_tensor_and_model_stream():
    """Single-rank RCCL group: the real flat gradient tensor (a view into the torch-allocated state arena) goes
    through dist.all_reduce on the model's stream, and the split step (forward_backward -> all_reduce ->
    apply_update(1/world)) equals the fused step."""
    import torch
    import torch.distributed as dist
    from data.episode import Episode
    from fsmg.dist import EpisodeParallel
    from models.lstm_baseline import LSTMBaseline
    cfg = small_config()
    sup, qry = _episode(cfg, 2, 2, 1)
    ref = LSTMBaseline(dict(cfg)); ref.recover_or_init('')
    want = [ref.train(Episode(sup, qry)) for _ in range(3)]
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(free_port())
    dist.init_process_group('nccl', rank=0, world_size=1)
    try:
        m = LSTMBaseline(dict(cfg)); m.recover_or_init('')        # broadcasts the arena over RCCL (no-op for 1 rank)
        assert m.grad_tensor.is_cuda and m.grad_tensor.dtype == torch.float32
        got = []
        for step in range(3):
            m.forward_backward(sup, qry)
            if step == 0:                       # single collective on the compute stream
                with m.stream_context():
                    dist.all_reduce(m.grad_tensor, op=dist.ReduceOp.SUM)
            else:                               # bucketed, asynchronous, on the communication stream
                works = []
                for b, t in enumerate(m.grad_buckets):
                    with m.comm_context(b):
                        works.append(dist.all_reduce(t, op=dist.ReduceOp.SUM, async_op=True))
                with m.stream_context():
                    for w in works:
                        w.wait()
            got.append(m.apply_update(1.0))
        assert got == want
        assert sum(t.numel() for t in m.grad_buckets) == m.grad_tensor.numel()
        assert EpisodeParallel(m).world == 1
    finally:
        dist.destroy_process_group()


def test_partitioned_order_at_hidden_1024_matches_the_oracle_at_cfg_c(monkeypatch):
    """The XCD-partitioned order at hidden 1024 (opt-in: measured to lose at cfg-C, profiles/r06_cfgC_xov_ab.txt) with every part on --
    the top layer's chains packed on three XCD pairs (15 rows each, four row groups), the gated projection beside the forward chain, dW
    beside the top BPTT chain, dK of layer 1 (two-part A, from the work queue) beside the BPTT chain of layer 0: loss and every gradient
    of a full cfg-C episode against the fp64 oracle, same bounds as the serial order; no time-out, and the order was really taken."""
    monkeypatch.setenv('FSMG_XCD_OVERLAP', '1')
    monkeypatch.setenv('FSMG_XOV_PARTS', '7')
    over, N, K, Q = FULL['cfg-C']
    cfg = small_config(**over)
    (sup, qry), = O.synthetic_episodes(1, N, K, Q, cfg['max_len'], cfg['input_size'], seed=8, realistic=True)
    model = new_model(cfg, max_sequences=N * (K + Q))
    params = f64_params(model)
    loss, cache, grads, aux = cached_oracle_step(('full', 'cfg-C'), params, sup, qry, cfg)
    for _ in range(2):                                          # (the second pass: queue words and inboxes left by the first)
        model.forward_backward(sup, qry)
        tail = model.debug_read('tail', 16)
        assert abs(tail[1] - loss) <= NLL_RTOL * abs(loss)
        for name_ in grads:
            assert rel_max(model.get_grad(name_), grads[name_]) < 2e-4, name_
    st = model.stats()
    assert st['timeouts'] == 0 and model.debug_read('xcd_bx3', 1)[0] == 1.0
    part = model.debug_read('xcd_partitioned', 3)
    assert part[0] == 1.0 and part[1] == 6.0 and part[2] == 1.0     # the passes took the partitioned order, chains on XCDs 0-5


@pytest.mark.parametrize('name', sorted(FULL))
def test_full_size_gradients_match_oracle(name, gemm_kind):
    """One full train episode of every BASELINE config that fits one GPU -- cfg-B (B=45, T=128, V1=10001, H=512),
    cfg-C (T=50, H=1024, L=2: the all-row-tiles forward kernel, k_lstm_bwd_rs<8>, the inter-layer dx path) and cfg-D
    (B=100: 7 row tiles) -- loss and EVERY gradient tensor vs the fp64 oracle (231 / 249 / 513 GFLOP in numpy),
    then one clip + Adam update, realistic Zipf/padded tokens."""
    over, N, K, Q = FULL[name]
    cfg = small_config(**over)
    (sup, qry), = O.synthetic_episodes(1, N, K, Q, cfg['max_len'], cfg['input_size'], seed=8, realistic=True)
    model = new_model(cfg, max_sequences=N * (K + Q))          # cfg-D (100 rows): the bf16-split XCD-local recurrence
    params = f64_params(model)
    loss, cache, grads, aux = cached_oracle_step(('full', name), params, sup, qry, cfg)
    params = {k: v.copy() for k, v in params.items()}
    model.forward_backward(sup, qry)
    tail = model.debug_read('tail', 16)
    assert abs(tail[1] - loss) <= NLL_RTOL * abs(loss)
    assert abs(tail[0] - aux['embedding_slices_sq']) <= 1e-4 * aux['embedding_slices_sq']
    for name_ in grads:
        assert rel_max(model.get_grad(name_), grads[name_]) < 2e-4, name_
    # element-wise on the embedding gradient (the max-norm above is blind to one wrong small row, e.g. a rare token's): rows of tokens
    # that do not occur are exact zeros, and every element of the rows that do is within 2e-4 of its own value plus 1e-6 of the
    # tensor's largest element (the heavy rows -- padding, START -- are sums over ~1000 positions and set that maximum; a rare token's
    # row is 1e-3 .. 1e-4 of it, so this floor still sees a wrong rare row where the max-norm's 2e-4 of the maximum is the size of the
    # row itself.  Measured worst: 2.1e-7 of the maximum, on a heavily cancelling element of the padding row)
    got_e, want_e = model.get_grad('embedding').astype(np.float64), grads['embedding']
    used = np.zeros(want_e.shape[0], bool)
    used[np.unique(cache['X'])] = True
    assert not got_e[~used].any() and not want_e[~used].any()
    err = np.abs(got_e[used] - want_e[used])
    bound = 2e-4 * np.abs(want_e[used]) + 1e-6 * np.abs(want_e).max()
    worst = np.unravel_index(np.argmax(err / bound), err.shape)
    assert (err <= bound).all(), ('embedding row %d' % np.flatnonzero(used)[worst[0]], err[worst], bound[worst], want_e[used][worst])
    got = model.apply_update(1.0)
    opt = O.new_opt_state(params)
    O.apply_update(params, grads, aux, opt, cfg)
    # one Adam step: the update is sign-like, m / (sqrt(v) + eps) = g / (|g| + 1e-8), so it amplifies the gradient's error where |g| ~ eps --
    # the bottom layer's bias at T = 128 under two layers (gate-gradient sums of ~1e-8): 2.9e-4 measured there, <= 1e-4 everywhere else
    upd_tol = 5e-4 if name == 'cfg-C-T128' else 1e-4
    for name_, ref in params.items():
        assert rel_max(model.get_param(name_), ref) < upd_tol, name_
    assert abs(got - loss) <= NLL_RTOL * abs(loss)


def test_lr_decay_is_exercised_from_a_resumed_step():
    """exponential_decay (reference src/models/lstm_baseline.py:77-81): lr_s = lr * 0.5 ** (global_step / n_decay),
    continuous, global_step read BEFORE the update.  n_decay = 3 and a counter resumed at 7 make the factor
    0.198 -> 0.025 over the ten updates: a wrong base, exponent or off-by-one moves the parameters by 20 %+ of an update,
    far outside the tolerance (every other test uses n_decay = 10000, a factor 0.9993)."""
    cfg = small_config(hidden_size=40, embedding_size=20, input_size=211, max_len=12, n_decay=3, lr=2e-2)
    model = new_model(cfg)
    params = f64_params(model)
    start = {k: v.copy() for k, v in params.items()}
    opt = O.new_opt_state(params)
    # global_step drives the decay AND Adam's bias correction (TF's beta powers are beta ** global_step for this
    # trainer: one apply_gradients per step); the slots start at zero here, as after set_step on a fresh handle
    model.step = 7
    opt['step'] = 7
    for s in range(10):
        sup, qry = _episode(cfg, 3, 3, 2, seed=300 + s)
        want = O.train_step(params, opt, sup, qry, cfg)
        got = model.train_step(sup, qry)
        assert abs(got - want) <= NLL_RTOL * abs(want), (s, got, want)
    assert model.step == 17
    moved = max(rel_max(params[k], start[k]) for k in params)
    for name, ref in params.items():
        assert rel_max(model.get_param(name), ref) < 5e-4, name
    assert moved > 0.02          # the parameters moved by far more than the tolerance: the check has teeth


def test_maml_step_and_eval_match_oracle_at_the_baseline_size():
    """cfg-E at BASELINE.json's own size -- freemidi vocabulary (V = 4708), 2-layer LSTM h = 1024, T = 50, 5-way / 5-shot /
    4 query, one inner clipped-SGD step of 0.1 (config/maml_lstm.yaml) -- one few-shot evaluation and one outer step against
    the fp64 oracle: query NLL at the adapted parameters, every parameter after clip + Adam, theta restored by the evaluation."""
    over, N, K, Q, inner_steps, inner_lr = FULL_E
    cfg = small_config(**over)
    (sup, qry), (sup2, qry2) = O.synthetic_episodes(2, N, K, Q, cfg['max_len'], cfg['input_size'], seed=43, realistic=True)
    model = new_model(cfg)
    params = f64_params(model)
    opt = O.new_opt_state(params)
    want_eval = O.maml_eval(params, sup2, qry2, cfg, inner_steps, inner_lr)
    got_eval = model.maml_eval(sup2, qry2, inner_steps, inner_lr)
    assert abs(got_eval - want_eval) <= NLL_RTOL * abs(want_eval), (got_eval, want_eval)
    for name, ref in params.items():                                    # evaluation left theta alone
        assert rel_max(model.get_param(name), ref) == 0.0, name
    want = O.maml_step(params, opt, sup, qry, cfg, inner_steps, inner_lr)
    got = model.maml_step(sup, qry, inner_steps, inner_lr)
    assert abs(got - want) <= NLL_RTOL * abs(want), (got, want)
    assert model.step == 1
    for name, ref in params.items():
        assert rel_max(model.get_param(name), ref) < 1e-4, name          # one Adam step from zero slots (sign-like update)


def test_ten_consecutive_train_losses_at_cfg_b():
    """The reference's own regression test (src/train/test_seed.py:17-65: N_UPDATES = 10 consecutive train losses from a
    fixed initialisation) at the headline workload's FULL size (cfg-B: V1 = 10001, T = 128, B = 45, H = 512): each of ten
    consecutive train losses within 1e-4 relative of the fp64 oracle started from the same parameters, a fresh episode per
    step, clip + Adam applied in between (BASELINE.md section 3 / SURVEY.md 8d parity gate)."""
    over, N, K, Q = FULL['cfg-B']
    cfg = small_config(**over)
    eps = O.synthetic_episodes(10, N, K, Q, cfg['max_len'], cfg['input_size'], seed=77, realistic=True)
    model = new_model(cfg)
    params = f64_params(model)
    opt = O.new_opt_state(params)
    worst = 0.0
    for s_, (sup, qry) in enumerate(eps):
        want = O.train_step(params, opt, sup, qry, cfg)
        got = model.train_step(sup, qry)
        worst = max(worst, abs(got - want) / abs(want))
        assert abs(got - want) <= NLL_RTOL * abs(want), (s_, got, want)
    assert model.step == 10
    print('ten full-size cfg-B train losses: worst relative error %.2e' % worst)


def test_ten_consecutive_train_losses_on_the_bf16_split_chain_at_cfg_d_rows():
    """The same ten-loss trajectory on cfg-D's episode shape (20-way, 1-shot, 4 query songs: 100 sequences, hidden 512): the
    bf16-split XCD-local recurrence with four row groups, the family cfg-D really runs (half the time steps of cfg-D to keep the
    fp64 oracle to seconds; the recurrence's arithmetic does not depend on T)."""
    over, N, K, Q = FULL['cfg-D']
    cfg = small_config(**dict(over, max_len=64))
    eps = O.synthetic_episodes(10, N, K, Q, cfg['max_len'], cfg['input_size'], seed=78, realistic=True)
    model = new_model(cfg, max_sequences=N * (K + Q))
    assert bool(model.debug_read('xcd_bx3', 1)[0])
    params = f64_params(model)
    opt = O.new_opt_state(params)
    for s_, (sup, qry) in enumerate(eps):
        want = O.train_step(params, opt, sup, qry, cfg)
        got = model.train_step(sup, qry)
        assert abs(got - want) <= NLL_RTOL * abs(want), (s_, got, want)
    st = model.stats()
    assert model.step == 10 and st['timeouts'] == 0 and st['xcd_launches'] > 0


FORCED = [(env, i) for env in ({'FSMG_XCD_BX3': '1'}, {'FSMG_GEMM_H': '2'}, {'FSMG_XCD_OVERLAP': '0'}) for i in (2, 4, 9, 10, 11, 12)] + [({'FSMG_GEMM_H': '2'}, 20)] + \
         [({'FSMG_XCD_OVERLAP': '1'}, i) for i in (9, 10)] + \
         [({'FSMG_XCD': '0'}, i) for i in (8, 16)] + \
         [({'FSMG_XCD_BX3': '1'}, 13), ({'FSMG_XCD_BX3': '1', 'FSMG_XCD_VARIANT': '32'}, 13), ({'FSMG_XCD_BX3': '1', 'FSMG_XCD_VARIANT': '176'}, 13)]
         # ... the XCD-partitioned order at shapes AUTO finds too small for it; the column-split persistent kernels at hidden 256 / 512; hidden 1024 on the
         # bf16 matrix pipe (k_lstm_*_pair16) where AUTO keeps the fp32 pair kernels (4 rows), with its default variants, with none of them
         # (32: every poll fetches all 24 fragments, write-through partials everywhere, early reset wait) and with probe but no streamed fetch (176)


@pytest.mark.parametrize('env,idx', FORCED, ids=['%s-%d' % ('+'.join(k + '=' + v for k, v in e.items()), i) for e, i in FORCED])
def test_forced_kernel_families_on_a_reduced_shape_list(env, idx, monkeypatch):
    """The kernel families a default run only picks at some shapes, forced at a reduced list of SHAPES (B = 45 rows, two stacked
    layers, hidden 512 with 1 / 2 / 4 row groups and stacked): the bf16-split XCD-local recurrence (FSMG_XCD_BX3=1), the
    256 x 256-tile GEMM wherever it can run (FSMG_GEMM_H=2), the serial order where AUTO would take the XCD-partitioned one
    (FSMG_XCD_OVERLAP=0) -- loss, h, c and every gradient against the fp64 oracle, same bounds as the default families.
    Every knob here is read by fsmg_create and stays with the handle, and the handle reports what it then ran: a case whose
    family did not run fails, however good its numbers are (tests/test_gemm_forced.py takes FSMG_GEMM_H=2 to the tile edges)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    over, N, K, Q = SHAPES[idx]
    cfg = small_config(**over)
    sup, qry = _episode(cfg, N, K, Q, seed=3)
    model = new_model(cfg, max_sequences=N * (K + Q))
    params = f64_params(model)
    loss, cache, grads, aux = cached_oracle_step(('shape', repr(sorted(over.items())), N, K, Q), params, sup, qry, cfg)
    B = N * (K + Q)
    model.forward_backward(sup, qry)
    d, L = model.debug_dims(), cfg['n_layers']
    if env.get('FSMG_GEMM_H') == '2':
        # [fp32 MFMA, k_gemm_bx3, k_gemm_bx3w, k_gemm_bx3h] launches of this first pass.  use_h_gemm (api_schedule.hip) declines by rule a
        # lane with lds_pad (the two-stream order's auxiliary lane: no shape here takes that order, V1 < 8 H L), a work-queue launch
        # (xcd_first: the XCD-partitioned order, off here) and an x-contiguous A that is gathered and not the first part of a merged
        # dK.  Of the 3 + 4 L GEMMs of a pass -- projection, dH, dW and per layer zx, dKh, dKx, dx -- the last rule meets exactly
        # one: dKx of layer 0 (embedding rows by token id), which falls to k_gemm_bx3 (use_ws_gemm's default rule wants 256 128-tiles),
        # unless Ep % 256 == 0 makes it the first part of the merged dKx + dKh GEMM (api_backward.hip dk_gemm).  zx of layer 0 gathers
        # K-contiguous rows, which the 256-tile kernel takes.  A layer above 0 with Hp % 256 == 0 merges its pair too.
        merged = [(d['Ep'] if l == 0 else d['Hp']) % 256 == 0 for l in range(L)]
        kinds = [int(x) for x in model.debug_read('gemm_kinds', 4)]
        assert kinds[3] > 0
        assert kinds == [0, 0 if merged[0] else 1, 0, 3 + 4 * L - sum(merged) - (0 if merged[0] else 1)]
        assert model.debug_read('fused_softmax', 2)[1] == 1          # dW on the 256-tile kernel: the pass took the fused softmax
        if idx == 20:
            # the merged dK ran (in_p = Ep = 256): with FSMG_MERGE_DK=0 on a second handle the same pass has one launch more, and it
            # is the gathered dKx on k_gemm_bx3
            assert merged == [True] and kinds == [0, 0, 0, 6]
            monkeypatch.setenv('FSMG_MERGE_DK', '0')
            pair = new_model(cfg, max_sequences=B)
            pair.forward_backward(sup, qry)
            assert [int(x) for x in pair.debug_read('gemm_kinds', 4)] == [0, 1, 0, 6]
    if 'FSMG_XCD_BX3' in env:        # (a no-op at hidden 48 / 32, shapes 2 and 4: only the XCD-local kernels of hidden 512 / 1024 have the format)
        assert bool(model.debug_read('xcd_bx3', 1)[0]) == (d['Hp'] in (512, 1024))
    if 'FSMG_XCD_OVERLAP' in env:    # whether this pass took the XCD-partitioned order
        assert model.debug_read('xcd_partitioned', 3)[2] == float(env['FSMG_XCD_OVERLAP'] == '1')
    if env.get('FSMG_XCD') == '0':
        st = model.stats()
        assert st['xcd_launches'] == 0 and st['persistent_launches'] > 0
    tail = model.debug_read('tail', 16)
    assert abs(tail[1] - loss) <= NLL_RTOL * abs(loss)
    for l in range(cfg['n_layers']):
        hs, cs, _ = read_states(model, cfg, l, B)
        assert rel_max(hs, cache['layers'][l]['hs']) < 2e-5 and rel_max(cs, cache['layers'][l]['cs']) < 2e-5, 'layer %d' % l
    for name in grads:
        assert rel_max(model.get_grad(name), grads[name]) < 2e-4, name
    assert abs(tail[0] - aux['embedding_slices_sq']) <= 1e-4 * aux['embedding_slices_sq']
    opt = O.new_opt_state(params)
    O.apply_update(params, grads, aux, opt, cfg)
    assert abs(model.apply_update(1.0) - loss) <= NLL_RTOL * abs(loss)
    for name, ref in params.items():
        assert rel_max(model.get_param(name), ref) < 5e-4, name


@pytest.mark.parametrize('kind', ['bx3', 'f32'])
def test_non_finite_weights_give_nan_with_the_bf16_split_and_inf_with_the_fp32_mfma(kind, monkeypatch):
    """Edge of the default GEMM (csrc/gemm.hip, "fp32 GEMM on the bf16 matrix pipe"), pinned as MEASURED on gfx950: an Inf
    operand makes the second piece of the split NaN (a2 = bf16(Inf - Inf)), so the logits it feeds are NaN where the fp32 MFMA
    (FSMG_GEMM=f32) produces +-Inf; a FINITE weight above bf16's largest value (3.395e38 > 3.39e38) still gives finite, huge
    logits with both kernels.  The damage stays in the column the bad weight feeds: every other logit keeps its bits, and an
    Inf weight never yields a finite loss (no silent garbage)."""
    monkeypatch.setenv('FSMG_GEMM', kind)
    cfg = small_config(hidden_size=32, embedding_size=16, input_size=130, max_len=5)
    sup, qry = _episode(cfg, 3, 2, 2, seed=5)
    B, T, V1 = 3 * 4, cfg['max_len'], cfg['input_size'] + 1
    clean = new_model(cfg)
    clean.debug_set('inplace_dlogits', 0)
    clean.forward_backward(sup, qry)
    V1p = clean.debug_dims()['V1p']
    ref = clean.debug_read('logits', B * T * V1p).reshape(B * T, V1p)[:, :V1].copy()
    for bad in (np.float32(np.inf), np.float32(3.395e38)):
        model = new_model(cfg)
        w = model.get_param('softmax_w')
        w[:, 7] = 0.0
        w[3, 7] = bad                                   # column 7 of the logits = bad * h[:, 3] (+ bias)
        model.set_param('softmax_w', w)
        model.debug_set('inplace_dlogits', 0)
        model.forward_backward(sup, qry)
        logits = model.debug_read('logits', B * T * V1p).reshape(B * T, V1p)[:, :V1]
        col = logits[:, 7]
        if np.isinf(bad):
            if kind == 'bx3':
                assert np.isnan(col).all()
            else:
                assert np.isinf(col).all() and not np.isnan(col).any()
            assert not np.isfinite(model.debug_read('tail', 16)[1])
        else:
            assert np.isfinite(col).all() and np.abs(col).max() > 1e30
        others = np.delete(logits, 7, axis=1)
        np.testing.assert_array_equal(others, np.delete(ref, 7, axis=1))


def test_library_owned_exchange_with_one_rank_equals_the_fused_step():
    """fsmg_comm_* (include/fsmg.h): with a communicator attached the library runs forward + backward -> ncclAllReduce of the
    three gradient buckets on its own communication stream -> clip + Adam (1 / world) inside fsmg_train_step.  One rank is all
    a 1-GPU box can form (RCCL refuses two ranks on one device), and with one rank the exchange must change nothing: the same
    bits as the single-graph step, for the plain step, the indexed step and the MAML-style step; the state broadcast and the
    release leave the handle usable."""
    from fsmg.binding import FsmgModel
    cfg = small_config(hidden_size=512, embedding_size=24, input_size=300, max_len=9, max_grad_norm=0.5)
    eps = O.synthetic_episodes(6, 5, 5, 4, cfg['max_len'], cfg['input_size'], seed=91, realistic=True)
    plain = new_model(cfg)
    want = [plain.train_step(s_, q_) for s_, q_ in eps[:3]] + [plain.maml_step(s_, q_, 1, 0.2) for s_, q_ in eps[3:5]]
    lib = new_model(cfg)
    lib.comm_init(FsmgModel.comm_unique_id(), 1, 0)
    lib.comm_broadcast_state(0)
    got = [lib.train_step(s_, q_) for s_, q_ in eps[:3]] + [lib.maml_step(s_, q_, 1, 0.2) for s_, q_ in eps[3:5]]
    assert got == want
    for name in plain.param_shapes:
        np.testing.assert_array_equal(lib.get_param(name), plain.get_param(name))
    assert lib.step == plain.step == 5
    lib.comm_release()
    assert lib.train_step(*eps[5]) == plain.train_step(*eps[5])


@pytest.mark.gpu
@pytest.mark.parametrize('layers,hidden', [(1, 512), (2, 64)])
def test_split_backward_cut_points_give_the_same_gradients_and_updates(layers, hidden):
    """fsmg_config.dp_split_backward (include/fsmg.h): the backward pass of the episode-parallel order replayed as two graphs,
    cut behind the projection gradients (1) or behind the last recurrent chain (2), so that bucket 0 of the gradient exchange
    can travel beside the second graph.  Where the cut sits changes when kernels are enqueued, never what they compute: every
    gradient tensor, three updates and the losses are bit-identical to the one-graph pass (0)."""
    cfg = small_config(hidden_size=hidden, embedding_size=24, input_size=300, max_len=9, max_grad_norm=0.5, n_layers=layers)
    eps = O.synthetic_episodes(3, 5, 5, 4, cfg['max_len'], cfg['input_size'], seed=17, realistic=True)
    ref = new_model(cfg)
    want_g, want_l = [], []
    for s_, q_ in eps:
        ref.forward_backward(s_, q_)
        want_g.append({k: ref.get_grad(k).copy() for k in ref.param_shapes})
        want_l.append(ref.apply_update(1.0))
    for mode in (1, 2):
        m = new_model(cfg, dp_split_backward=mode)
        for i, (s_, q_) in enumerate(eps):
            m.forward_backward(s_, q_)
            for k in m.param_shapes:
                np.testing.assert_array_equal(m.get_grad(k), want_g[i][k], err_msg='cut %d, step %d, %s' % (mode, i, k))
            assert m.apply_update(1.0) == want_l[i]
        for k in ref.param_shapes:
            np.testing.assert_array_equal(m.get_param(k), ref.get_param(k))


@pytest.mark.parametrize('over,N,K,Q', [
    (dict(hidden_size=64, embedding_size=16, input_size=130, max_len=7), 3, 2, 2),      # three-pass cross entropy kernel? no: register kernel, 6 float4 per thread
    (dict(hidden_size=32, embedding_size=16, input_size=7000, max_len=4), 2, 2, 1),     # 12 float4 per thread
    (dict(hidden_size=32, embedding_size=16, input_size=13000, max_len=3), 2, 1, 1),    # rows past 12 * 1024 floats: the three-pass kernel
])
def test_inplace_dlogits_gives_the_same_bits(over, N, K, Q):
    """Round 5: a train pass's cross entropy writes dlogits over the logits it has just read (one buffer instead of two; default).
    Every row is in registers (or re-read by the thread that overwrites it) before the first store: dlogits and every gradient
    carry the same bits as with two buffers, for each of the three cross-entropy kernels."""
    cfg = small_config(**over)
    sup, qry = _episode(cfg, N, K, Q, seed=11)
    a, b = new_model(cfg), new_model(cfg)
    b.debug_set('inplace_dlogits', 0)
    a.debug_set('fused_softmax', 0)                 # (these shapes never take it; said so that the test keeps meaning what it says)
    a.forward_backward(sup, qry); b.forward_backward(sup, qry)
    d = a.debug_dims()
    n = N * (K + Q) * d['T'] * d['V1p']
    np.testing.assert_array_equal(a.debug_read('dlogits', n), b.debug_read('dlogits', n))
    np.testing.assert_array_equal(a.debug_read('logits', n), a.debug_read('dlogits', n))          # one buffer
    assert not np.array_equal(b.debug_read('logits', n), b.debug_read('dlogits', n))              # two
    for name in a.param_shapes:
        np.testing.assert_array_equal(a.get_grad(name), b.get_grad(name))
    assert a.apply_update(1.0) == b.apply_update(1.0)


def test_split_update_gives_the_same_bits_and_every_reader_waits_for_it():
    """Round 5 (fsmg_debug_set("upd_split", 1)): clip + Adam of an eager pass as two launches -- [embedding .. LSTM layers] on the main stream, [softmax_w, softmax_b]
    on the auxiliary stream beside the next step's input phase; the first publishes (go, clip scale, alpha), the second consumes
    them.  Same arithmetic: parameters, moments and losses are bit-identical to the single launch over six steps, a parameter read
    straight after a step sees the finished update (fsmg_host::begin_call settles the pending half), a step whose batch is
    rejected (token out of range) skips BOTH halves, and the episode-parallel pair forward_backward / apply_update splits too."""
    cfg = small_config(hidden_size=512, embedding_size=32, input_size=300, max_len=10)
    eps = O.synthetic_episodes(6, 5, 5, 4, cfg['max_len'], cfg['input_size'], seed=51)
    a, b = new_model(cfg, max_sequences=45), new_model(cfg, max_sequences=45)
    a.debug_set('upd_split', 1)                     # (not the default: measured slower, DESIGN.md 10 -- kept as a knob, and kept correct)
    b.debug_set('upd_split', 0)
    for i, (s_, q_) in enumerate(eps):
        if i == 3:                                  # the split forward_backward / apply_update pair in the middle
            a.forward_backward(s_, q_); b.forward_backward(s_, q_)
            assert a.apply_update(1.0) == b.apply_update(1.0)
        else:
            assert a.train_step(s_, q_) == b.train_step(s_, q_)
        if i in (0, 4):                             # read straight behind the step: no explicit synchronisation in between
            np.testing.assert_array_equal(a.get_param('softmax_w'), b.get_param('softmax_w'))
    bad = eps[0][0].copy(); bad[0, 0, 0] = cfg['input_size'] + 5
    before = a.get_param('softmax_b')
    with pytest.raises(Exception, match='TOKEN_RANGE'):
        a.train_step(bad, eps[0][1])
    np.testing.assert_array_equal(a.get_param('softmax_b'), before)                # the rejected batch touched neither half
    assert a.step == b.step == 6
    pa, pb = a.get_params(), b.get_params()
    for k in pa:
        np.testing.assert_array_equal(pa[k], pb[k])
    for k in pa:
        (ma, va), (mb, vb) = a.get_opt_state(k), b.get_opt_state(k)
        np.testing.assert_array_equal(ma, mb); np.testing.assert_array_equal(va, vb)
    assert abs(a.eval_step(eps[0][1]) - b.eval_step(eps[0][1])) == 0.0


def test_xov_selfcheck_passes_on_this_runtime_and_a_fault_parks_the_order(monkeypatch):
    """the gated projection of the XCD-partitioned order reads rows another XCD wrote mid-kernel with ordinary
    loads behind a relaxed poll -- correct only while no stale line of those rows sits in the consumer's L2, a property of the
    runtime, and a violation would be silent.  The first passes of every handle therefore recompute the logits on the serial path
    and compare the words (api_forward.hip xov_selfcheck).  Here: (1) on this ROCm / firmware the check passes -- zero differing
    words, the order stays on; (2) a forced fault (the comparison runs against a buffer that is not the recomputed logits) skips
    the step, repeats it, tallies the words, parks the order for the handle -- and the losses and parameters are those of a handle
    that ran the serial order all along on the same kernels."""
    monkeypatch.setenv('FSMG_XCD_OVERLAP', '1')
    cfg = small_config(hidden_size=512, embedding_size=32, input_size=3000, max_len=32)
    eps = O.synthetic_episodes(5, 5, 5, 4, cfg['max_len'], cfg['input_size'], seed=36)
    a = new_model(cfg, max_sequences=45)
    assert a.debug_read('xcd_partitioned', 2)[0] == 1.0
    a.debug_set('xov_selfcheck', 3)
    la = [a.train_step(*e) for e in eps[:3]]
    st = a.stats()
    assert st['xov_selfcheck_mismatches'] == 0 and st['timeouts'] == 0 and a.debug_read('xcd_partitioned', 3)[2] == 1.0
    a.debug_set('xov_selfcheck', 1); a.debug_set('xov_selfcheck_fault', 1); a.debug_set('fallback_steps', 2)
    la.append(a.train_step(*eps[3]))                 # skipped, repeated on per-step launches
    st = a.stats()
    assert st['xov_selfcheck_mismatches'] > 0 and st['steps_skipped_timeout'] == 1 and a.step == 4
    assert a.debug_read('xcd_partitioned', 1)[0] == 0.0                         # parked
    la.append(a.train_step(*eps[4]))
    assert int(a.debug_read('xcd_partitioned', 3)[2]) == 0
    monkeypatch.setenv('FSMG_XCD_OVERLAP', '0'); monkeypatch.setenv('FSMG_XCD_BX3', '1')
    b = new_model(cfg, max_sequences=45)
    lb = [b.train_step(*e) for e in eps[:3]]
    b.debug_set('persistent', 0); lb.append(b.train_step(*eps[3])); b.debug_set('persistent', 1)
    lb.append(b.train_step(*eps[4]))
    # forward passes are bit-identical across the orders; dW's K split differs under the partitioned order: later losses to rounding
    assert la[0] == lb[0]
    np.testing.assert_allclose(la, lb, rtol=2e-6)


def test_xov_selfcheck_comes_back_periodically_and_a_late_fault_parks_the_order(monkeypatch):
    """the self-check screened a handle's first two passes and then trusted the unfenced cross-XCD read forever.  It
    now also runs on one pass in every `xov_selfcheck_every` (default 1000) for the handle's whole life.  Here with a period of 3: passes
    1, 2 (the start-up screen), 3 and 6 are checked, 4 and 5 are not; a fault injected after pass 4 goes unnoticed on pass 5 (by design:
    that pass is not checked) and is caught on pass 6 -- the step is skipped, repeated, and the order parked for the handle."""
    monkeypatch.setenv('FSMG_XCD_OVERLAP', '1')
    cfg = small_config(hidden_size=512, embedding_size=32, input_size=3000, max_len=32)
    eps = O.synthetic_episodes(7, 5, 5, 4, cfg['max_len'], cfg['input_size'], seed=37)
    a = new_model(cfg, max_sequences=45)
    assert a.debug_read('xcd_partitioned', 2)[0] == 1.0 and a.debug_read('xov_selfcheck', 3)[2] == 1000.0      # the default period
    a.debug_set('xov_selfcheck_every', 3)
    for e in eps[:4]:
        a.train_step(*e)
    assert [int(v) for v in a.debug_read('xov_selfcheck', 3)] == [3, 4, 3]
    st = a.stats()
    assert st['xov_selfcheck_mismatches'] == 0 and st['timeouts'] == 0
    a.debug_set('xov_selfcheck_fault', 1); a.debug_set('fallback_steps', 2)
    a.train_step(*eps[4])                            # pass 5: not a checked pass
    assert a.stats()['xov_selfcheck_mismatches'] == 0 and int(a.debug_read('xov_selfcheck', 3)[0]) == 3
    a.train_step(*eps[5])                            # pass 6: checked -- skipped, repeated on per-step launches, parked
    st = a.stats()
    assert st['xov_selfcheck_mismatches'] > 0 and st['steps_skipped_timeout'] == 1 and a.step == 6
    assert a.debug_read('xcd_partitioned', 1)[0] == 0.0 and int(a.debug_read('xov_selfcheck', 3)[0]) == 4
    assert np.isfinite(a.train_step(*eps[6])) and a.step == 7 and int(a.debug_read('xcd_partitioned', 3)[2]) == 0


@pytest.mark.parametrize('hidden,layers', [(512, 1), (1024, 2)])
def test_lazy_column_split_copies_are_refreshed_before_anybody_reads_them(hidden, layers, monkeypatch):
    """Round 5: a handle whose passes take the XCD-local kernels refreshes only their register images behind an update; the
    column-split fragment copies of K_h go stale until a pass is about to read them (ensure_cs): a validation batch too large for
    the XCD-local kernels, the per-step fallback, a forced column-split run.  Against a handle that refreshes both layouts every
    time (FSMG_LAZY_CS=0): the same bits everywhere."""
    cfg = small_config(hidden_size=hidden, embedding_size=16, input_size=60, max_len=5, n_layers=layers)
    eps = O.synthetic_episodes(5, 3, 2, 2, cfg['max_len'], cfg['input_size'], seed=61)
    a = new_model(cfg)
    monkeypatch.setenv('FSMG_LAZY_CS', '0')
    b = new_model(cfg)
    monkeypatch.delenv('FSMG_LAZY_CS')
    for e in eps[:2]:
        assert a.train_step(*e) == b.train_step(*e)
    assert a.stats()['xcd_launches'] > 0
    big = np.random.RandomState(3).randint(0, cfg['input_size'], size=(16, 3, 3, cfg['max_len'])).astype(np.int32)      # 144 rows per pass
    np.testing.assert_array_equal(a.eval_batch(big), b.eval_batch(big))                  # per-step / column-split kernels read khf
    assert a.train_step(*eps[2]) == b.train_step(*eps[2])                                # stale again behind this update ...
    a.debug_set('persistent', 0); b.debug_set('persistent', 0)
    assert a.train_step(*eps[3]) == b.train_step(*eps[3])                                # ... and read by the per-step kernels
    a.debug_set('persistent', 1); b.debug_set('persistent', 1)
    assert a.train_step(*eps[4]) == b.train_step(*eps[4])
    for k, v in b.get_params().items():
        np.testing.assert_array_equal(a.get_param(k), v)


def test_every_handle_of_a_process_gets_a_second_stream_that_runs_beside_its_own():
    """Round 5: with five or more handles alive in a process, handles 5, 7 and 9 ran 1.68 -> 2.49 ms per cfg-B step -- silently,
    every kernel 15-60 us longer -- as soon as a step touched their lowest-priority auxiliary stream (profiles/r05_hw_queue_probe.txt).
    The auxiliary stream has the default priority now (nothing lost: same file), and since both streams of a handle then share one
    pool of hardware queues fsmg_create probes that the pair really overlaps (a wave on the main stream polls a flag a kernel on the
    candidate sets) and draws another stream otherwise.  Ten live handles: each has its second stream, their step times agree."""
    import time
    import torch
    over, N, K, Q = FULL['cfg-B']
    cfg = small_config(**dict(over, max_len=32))
    eps = O.synthetic_episodes(2, N, K, Q, cfg['max_len'], cfg['input_size'], seed=91)
    models, tries, ms = [], [], []
    for i in range(10):
        m = new_model(cfg, max_sequences=N * (K + Q))
        models.append(m)
        tries.append(int(m.debug_read('aux_tries', 1)[0]))
        for _ in range(4):
            m.train_step(*eps[0])
        m.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            m.train_step(*eps[1], want_loss=False)
        m.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0) / 10)
    assert all(t >= 1 for t in tries), tries
    assert max(ms) < 1.25 * min(ms), (ms, tries)            # a serialised pair is +45 % at this shape
    assert all(m.stats()['timeouts'] == 0 for m in models)
    # the probe's outcome is part of fsmg_stats, and asking again on a handle that has its stream changes nothing
    assert [m.stats()['aux_stream_tries'] for m in models] == tries
    models[0].debug_set('reprobe_aux', 1)
    assert models[0].stats()['aux_stream_tries'] == tries[0] and np.isfinite(models[0].train_step(*eps[0]))


def test_handles_of_one_process_take_turns_on_the_device():
    """Calls return before their work is done, and the persistent kernels of a pass -- recurrence chains, gated work-queue GEMMs -- spin
    on CUs they hold: two handles whose passes overlapped on the GPU would time-share those CUs at best and trip the hand-off time-out at
    worst.  A call of one handle that follows a call of another on the same device therefore orders itself behind what that one had
    issued (take_turn, csrc/api_handle.hip).  Three cfg-B handles stepped
    round-robin WITHOUT a synchronize in between: no time-out, and every handle's losses and parameters are bit for bit those of the
    same handle stepped alone."""
    over, N, K, Q = FULL['cfg-B']
    cfg = small_config(**dict(over, max_len=64))
    eps = O.synthetic_episodes(4, N, K, Q, cfg['max_len'], cfg['input_size'], seed=93)

    def make(i):
        return new_model(dict(cfg, seed=3 + i), max_sequences=N * (K + Q))
    alone = []
    for i in range(3):
        m = make(i)
        for s_ in range(6):
            m.train_step(*eps[(i + s_) % 4], want_loss=False)
        alone.append({k: m.get_param(k).copy() for k in m.param_shapes})
        m.close()
    models = [make(i) for i in range(3)]
    for s_ in range(6):
        for i, m in enumerate(models):
            m.train_step(*eps[(i + s_) % 4], want_loss=False)        # nothing waits for the GPU here
            if i == 1:
                m.debug_set('fallback_steps', 200)                   # (a cheap entry point between two passes takes its turn too)
    for i, m in enumerate(models):
        st = m.stats()
        assert st['timeouts'] == 0 and st['steps_skipped_timeout'] == 0 and m.step == 6, (i, st)
        for k, v in alone[i].items():
            np.testing.assert_array_equal(m.get_param(k), v)


REF_DEFAULT = (dict(input_size=10000, max_len=50, embedding_size=250, hidden_size=200, n_layers=1), 5, 5, 4)       # the reference's shipped dims


@pytest.mark.parametrize('name,order', [('cfg-B', 'partitioned'), ('cfg-B', 'serial'), ('ref-default', 'serial'), ('cfg-C', 'serial')])
def test_fused_softmax_matches_the_cross_entropy_pass(name, order, monkeypatch):
    """Round 5: where the projection's weight gradient runs on the 256 x 256-tile kernel a train pass never materialises
    (softmax - onehot) / n: the projection's epilogue stores E = exp(logit) and per-slice partials, k_ce_finish derives lse, the loss,
    c_r = 1 / (n S_r), patches E[r][y_r] -= S_r and writes c_r h_r; dH = diag(c) (E' W^T), dW = (diag(c) Hout)^T E', dd = the c-weighted
    column sums of E'.  Against the same handle configuration with the cross-entropy pass (fused_softmax = 0), cfg-B full size, in the
    XCD-partitioned and in the serial order: losses to 2e-6, lse / ce to 1e-6, every gradient to 2e-5 of its largest element, three
    updates on -- and against the fp64 oracle inside the tolerances of every other full-size test.  The projection itself may be any of
    the bf16-split kernels (one epilogue): the 128-tile ones at the reference's shipped dims and at cfg-C (two layers of 1024)."""
    monkeypatch.setenv('FSMG_XCD_OVERLAP', '1' if order == 'partitioned' else '0')
    over, N, K, Q = REF_DEFAULT if name == 'ref-default' else FULL[name]
    cfg = small_config(**over)
    B, T = N * (K + Q), cfg['max_len']
    eps = O.synthetic_episodes(4, N, K, Q, T, cfg['input_size'], seed=101)
    a, b = new_model(cfg, max_sequences=B), new_model(cfg, max_sequences=B)
    b.debug_set('fused_softmax', 0)
    a.forward_backward(*eps[0]); b.forward_backward(*eps[0])
    assert list(a.debug_read('fused_softmax', 2)) == [1.0, 1.0] and list(b.debug_read('fused_softmax', 2)) == [0.0, 0.0]
    np.testing.assert_allclose(a.debug_read('lse', B * T), b.debug_read('lse', B * T), rtol=1e-6)
    np.testing.assert_allclose(a.debug_read('ce', B * T), b.debug_read('ce', B * T), rtol=1e-5, atol=1e-6)
    for k in a.param_shapes:
        ga, gb = a.get_grad(k), b.get_grad(k)
        assert np.abs(ga - gb).max() <= 2e-5 * np.abs(gb).max(), k
    params = f64_params(a)
    loss, cache, grads, aux = cached_oracle_step(('fused', name, order), params, eps[0][0], eps[0][1], cfg)
    for k in grads:
        assert rel_max(a.get_grad(k), grads[k]) < 2e-4, k
    la, lb = a.apply_update(1.0), b.apply_update(1.0)
    assert abs(la - lb) <= 2e-6 * abs(lb) and abs(la - loss) <= NLL_RTOL * abs(loss)
    for e in eps[1:]:
        la, lb = a.train_step(*e), b.train_step(*e)
        assert abs(la - lb) <= 5e-6 * abs(lb)
    st = a.stats()
    assert st['timeouts'] == 0 and st['softmax_range_rows'] == 0 and st['xov_selfcheck_mismatches'] == 0


@pytest.mark.parametrize('case', ['row_sum_overflows', 'target_underflows'])
def test_fused_softmax_falls_back_when_a_logit_leaves_its_range(case):
    """The fused softmax stores exp(logit) without a shift: fine while a row's sum of them stays within [e^-60, 1e30] (its largest
    logit within about [-60, 60]) and exp(target logit) >= 1e-30, checked per row by k_ce_finish.  A bias of 100 on one word puts every row outside: the step is skipped on the device (no update), repeated with
    the cross-entropy pass, and the handle keeps that pass from then on -- same losses as a handle that never used the fused form.
    A bias of -80 on half the vocabulary leaves the row sums alone but takes exp(target logit) of about half the rows below 1e-30."""
    over, N, K, Q = FULL['cfg-B']
    cfg = small_config(**dict(over, max_len=80))                       # 3600 rows: still on the 256 x 256-tile kernels
    eps = O.synthetic_episodes(3, N, K, Q, cfg['max_len'], cfg['input_size'], seed=102)
    a, b = new_model(cfg, max_sequences=N * (K + Q)), new_model(cfg, max_sequences=N * (K + Q))
    b.debug_set('fused_softmax', 0)
    la0, lb0 = a.train_step(*eps[0]), b.train_step(*eps[0])
    assert a.debug_read('fused_softmax', 2)[1] == 1.0 and abs(la0 - lb0) <= 5e-6 * abs(lb0)
    for m in (a, b):
        d = m.get_param('softmax_b')
        if case == 'row_sum_overflows': d[7] = 100.0
        else: d[:5000] = -80.0
        m.set_param('softmax_b', d)
    a.debug_set('fallback_steps', 1)
    la, lb = a.train_step(*eps[1]), b.train_step(*eps[1])
    st = a.stats()
    # its own cause with its own tally: nothing timed out, the persistent kernels stay in force, no fallback period starts
    assert st['softmax_range_rows'] > 0 and st['steps_skipped_softmax_range'] == 1 and a.step == b.step == 2
    assert st['steps_skipped_timeout'] == 0 and st['timeouts'] == 0 and st['persistent_path'] == 1 and st['fallback_steps_left'] == 0
    assert list(a.debug_read('fused_softmax', 2)) == [0.0, 0.0]
    assert abs(la - lb) <= 5e-6 * abs(lb)
    la, lb = a.train_step(*eps[2]), b.train_step(*eps[2])
    assert abs(la - lb) <= 2e-5 * abs(lb) and a.stats()['steps_skipped_softmax_range'] == 1
    # the split call sequence (episode-parallel path) reports the cause by status code, and the update it refused left the step alone
    from fsmg.binding import FsmgError
    c = new_model(cfg, max_sequences=N * (K + Q))
    c.set_param('softmax_b', a.get_param('softmax_b'))
    c.forward_backward(*eps[1])
    with pytest.raises(FsmgError) as ei:
        c.apply_update(1.0)
    assert ei.value.code == -10 and c.step == 0 and c.stats()['steps_skipped_softmax_range'] == 1
    c.forward_backward(*eps[1])
    assert np.isfinite(c.apply_update(1.0)) and c.step == 1
