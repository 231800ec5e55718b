"""fp64 restatement of the MAML-style step with per-song lengths (TEST INFRASTRUCTURE ONLY; numpy).

tests/masked_ref.py's loss and backward pass (masked_loss, masked_backward) inside the loop of tests/maml_ref.py::adapt_full:

    theta'_{i+1} = theta'_i - inner_lr * clip_by_global_norm(grad of L_sup(theta'_i), max_grad_norm)
    L_sup = sum over support (b, t < len[b]) of ce / (n_valid_sup + 1e-12)            one group of N*K rows
    outer gradient = grad of L_qry at theta', L_qry the same sum over the query rows / (n_valid_qry + 1e-12)

The oracle's order and its division forms are kept, so that with every length T the whole thing is oracle.lstm_oracle.maml_adapt /
maml_query_grads / maml_step / maml_eval bit for bit in fp64 (tests/test_maml_masked_cpu.py).

`wrong`: one of WRONG, the same computation with one planted mistake -- what the CPU file shows its checks to catch.
"""
import numpy as np

import masked_ref as KR
from oracle import lstm_oracle as O

WRONG = ('rows_times_T', 'query_lengths_on_support', 'lengths_dropped_on_step_2', 'padding_ids_in_embedding_grad')


def lengths_of(shape, T, seed_offset=0):
    """seeded (support_len [N,K], query_len [N,Q]) for a shape of maml_ref.MAML_SHAPES: every set of two rows or more holds a 1 and a
    T (masked_ref.lengths_for), a set of ONE row cannot hold both and gets one value strictly inside (1, T); the two sums differ, so
    that swapped arrays cannot pass"""
    over, N, K, Q, n, seed = shape
    for attempt in range(64):            # (seeded rejection: the first draw whose two sums and two means differ)
        rng = np.random.RandomState(2200 + seed + seed_offset + 1000 * attempt)

        def one(rows):
            if int(np.prod(rows)) == 1:
                return np.full(rows, rng.randint(2, T), np.int32)
            return KR.lengths_for(rng, rows, T)
        sl, ql = one((N, K)), one((N, Q))
        if int(sl.sum()) != int(ql.sum()) and int(sl.sum()) * ql.size != int(ql.sum()) * sl.size:
            return sl, ql
    raise AssertionError('no lengths with different sums for %r' % (shape,))


def _pass(params, tokens, lengths, config, wrong=None):
    """one masked forward + backward over `tokens` [.., T] with `lengths` -> (loss, grads, aux, cache)"""
    d = O.model_dims(config)
    X, Y = O.tokens_to_input_and_target(tokens, d['start'])
    lengths = np.asarray(lengths).reshape(-1)
    if wrong != 'padding_ids_in_embedding_grad':
        # the device's fixed ids behind a song's end (masked_ref.device_xy): the input is the start word, the target 0
        pad = np.arange(X.shape[1])[None, :] >= lengths[:, None]
        X, Y = X.copy(), Y.copy()
        X[pad], Y[pad] = d['start'], 0
    _, cache = O.forward(params, X, Y, config)
    if wrong == 'rows_times_T':
        T = d['T']
        mask = KR.mask_of(lengths, T).astype(cache['ce'].dtype)
        loss = (cache['ce'] * mask).sum() / (lengths.size * T + 1e-12)
        grads, aux = KR.masked_backward(params, cache, config, lengths)
        f = params['embedding'].dtype.type((int(lengths.sum()) + 1e-12) / (lengths.size * T + 1e-12))
        grads = {k: g * f for k, g in grads.items()}
        aux = dict(embedding_slices_sq=aux['embedding_slices_sq'] * float(f) ** 2)
        return float(loss), grads, aux, cache
    grads, aux = KR.masked_backward(params, cache, config, lengths)
    if wrong == 'padding_ids_in_embedding_grad':
        # the caller's ids at t >= len are read as inputs: the forward pass behind a song's end changes nothing that is scored, but
        # the embedding gradient files its (exactly zero) slices under those ids -- and a planted nonzero makes it visible
        n = X.size
        dx_pad = np.zeros((n, grads['embedding'].shape[1]), grads['embedding'].dtype)
        pad = (np.arange(X.shape[1])[None, :] >= lengths[:, None]).reshape(n)
        dx_pad[pad] = 1e-3
        np.add.at(grads['embedding'], X.reshape(n), dx_pad)
    return float(KR.masked_loss(cache, lengths, config)), grads, aux, cache


def adapt_full(params, support, support_len, config, inner_steps=1, inner_lr=0.1, clip_norm_mode='tf1_slices', wrong=None,
               query_len=None):
    """maml_ref.adapt_full with the masked support loss -> (theta', steps); steps[i] = dict(before = theta'_i, loss, grads, aux,
    gnorm, scale, theta = theta'_{i+1}).  fp64 parameters and full lengths give O.maml_adapt bit for bit."""
    assert wrong is None or wrong in WRONG, wrong
    fast = {k: v.copy() for k, v in params.items()}
    clip = float(config['max_grad_norm'])
    T = O.model_dims(config)['T']
    steps = []
    for i in range(int(inner_steps)):
        ln = np.asarray(support_len).reshape(-1)
        if wrong == 'query_lengths_on_support':
            ln = np.resize(np.asarray(query_len).reshape(-1), ln.size)
        if wrong == 'lengths_dropped_on_step_2' and i >= 1:
            ln = np.full(ln.size, T)
        loss, grads, aux, _ = _pass(fast, support, ln, config, wrong)
        gnorm = O.global_norm(grads, aux, clip_norm_mode)
        scale = clip / max(gnorm, clip)
        new = {}
        for k in fast:
            dt = fast[k].dtype.type
            new[k] = fast[k] - dt(inner_lr) * (grads[k] * dt(scale))
        steps.append(dict(before=fast, loss=loss, grads=grads, aux=aux, gnorm=gnorm, scale=scale, theta=new))
        fast = new
    return fast, steps


def query_grads(params, support, query, support_len, query_len, config, inner_steps=1, inner_lr=0.1, clip_norm_mode='tf1_slices',
                wrong=None):
    """-> dict(theta = theta', steps, loss = L_qry(theta'), grads = the first-order outer gradients, aux)"""
    fast, steps = adapt_full(params, support, support_len, config, inner_steps, inner_lr, clip_norm_mode, wrong, query_len)
    loss, grads, aux, _ = _pass(fast, query, query_len, config, wrong if wrong in ('rows_times_T', 'padding_ids_in_embedding_grad') else None)
    return dict(theta=fast, steps=steps, loss=loss, grads=grads, aux=aux)


def maml_step(params, opt, support, query, support_len, query_len, config, inner_steps=1, inner_lr=0.1, clip_norm_mode='tf1_slices'):
    """O.maml_step with the masked losses: mutates params / opt; returns L_qry(theta')"""
    r = query_grads(params, support, query, support_len, query_len, config, inner_steps, inner_lr, clip_norm_mode)
    O.apply_update(params, r['grads'], r['aux'], opt, config, clip_norm_mode)
    return r['loss']


def maml_eval(params, support, query, support_len, query_len, config, inner_steps=1, inner_lr=0.1, clip_norm_mode='tf1_slices',
              wrong=None):
    """O.maml_eval with the masked losses: adapt on the support rows' valid positions, the query rows' NLL over theirs"""
    fast, _ = adapt_full(params, support, support_len, config, inner_steps, inner_lr, clip_norm_mode, wrong, query_len)
    if wrong == 'rows_times_T':
        return _pass(fast, query, query_len, config, wrong)[0]
    return KR.eval_step(fast, query, query_len, config)
