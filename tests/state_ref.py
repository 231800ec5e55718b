"""A state pass (include/fsmg.h fsmg_*_state) restated in numpy (TEST INFRASTRUCTURE ONLY).

One segment of T tokens read from a carried state: import of h, c per layer, the pending token at position 0, the masked loss of one
group, gradients with the incoming state held constant, export at len[b], the context rule.  `dtype` float64 is the reference, float32
the measure of what fp32 arithmetic in this order costs (e32).  `mistake` plants ONE wrong-by-construction variant; the CPU tests
require each to move an asserted quantity of tests/test_gpu_state.py by more than twice that quantity's bound.
"""
import numpy as np

from oracle import lstm_oracle as O

MISTAKES = ('start_word', 'no_c', 'no_hprev_dk', 'export_T', 'swap_layers', 'table_start', 'grad_through_state')


def fresh_state(cfg, R, dtype=np.float64):
    d = O.model_dims(cfg)
    return dict(h=np.zeros((d['L'], R, d['H']), dtype), c=np.zeros((d['L'], R, d['H']), dtype),
                pending=np.full(R, d['start'], np.int64), ctx=np.zeros((R, 0), np.int64))


def device_xy(tokens, lengths, pending, start):
    """-> X, Y, mask [R, T]: what k_state_token_prep leaves (fixed ids behind a row's end, the pending token at position 0 of a row that
    has any scored position)"""
    tokens = np.asarray(tokens, np.int64)
    R, T = tokens.shape
    t = np.arange(T)[None, :]
    ln = np.asarray(lengths, np.int64)[:, None]
    mask = t < ln
    Y = np.where(mask, tokens, 0)
    X = np.empty_like(tokens)
    X[:, 1:] = np.where(t[:, 1:] < ln, tokens[:, :-1], start)
    X[:, 0] = np.where(ln[:, 0] > 0, np.asarray(pending, np.int64), start)
    return X, Y, mask


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def run(params, h0, c0, X, Y, W, cfg, want_grads=True, dk_hprev=True, emb_rows=None, f=None):
    """forward (+ backward) of R rows of any length from (h0, c0) [L, R, H] with per-position loss weights W [R, T]: loss = sum(W * ce).
    The state is a constant of the backward pass.  emb_rows: the embedding rows the input gradient is scattered to (default X).
    f: dropout factors per site, [L + 1] arrays [R, T, width] (tests/dropout_ref.py factors): non-recurrent sites only."""
    dt = params['embedding'].dtype
    d = O.model_dims(cfg)
    H, L = d['H'], d['L']
    R, T = X.shape
    W = np.asarray(W, dt)
    layer_in = params['embedding'][X]
    if f is not None:
        layer_in = layer_in * f[0].astype(dt)
    layers = []
    for l in range(L):
        K, b = params['kernel_%d' % l], params['bias_%d' % l]
        n_in = layer_in.shape[2]
        zx = layer_in.reshape(R * T, n_in).dot(K[:n_in]).reshape(R, T, 4 * H) + b
        h, c = h0[l].astype(dt), c0[l].astype(dt)
        hs, cs = np.zeros((T + 1, R, H), dt), np.zeros((T + 1, R, H), dt)
        hs[0], cs[0] = h, c
        gates = np.zeros((T, 4, R, H), dt)
        for t in range(T):
            z = zx[:, t] + h.dot(K[n_in:])
            si, tj = _sig(z[:, :H]), np.tanh(z[:, H:2 * H])
            sf, so = _sig(z[:, 2 * H:3 * H] + dt.type(O.FORGET_BIAS)), _sig(z[:, 3 * H:])
            c = c * sf + si * tj
            h = np.tanh(c) * so
            hs[t + 1], cs[t + 1] = h, c
            gates[t] = si, tj, sf, so
        layers.append(dict(x=layer_in, hs=hs, cs=cs, gates=gates))
        layer_in = np.transpose(hs[1:], (1, 0, 2))
        if f is not None:
            layer_in = layer_in * f[l + 1].astype(dt)
    out = layer_in.reshape(R * T, H)
    logits = out.dot(params['softmax_w']) + params['softmax_b']
    m = logits.max(axis=1)
    lse = m + np.log(np.exp(logits - m[:, None]).sum(axis=1))
    yf = Y.reshape(R * T)
    tgt = logits[np.arange(R * T), yf]
    ce = lse - tgt
    res = dict(loss=dt.type((W.reshape(-1) * ce).sum()), logprob=(tgt - lse).reshape(R, T), ce=ce.reshape(R, T),
               hs=np.stack([lay['hs'] for lay in layers]), cs=np.stack([lay['cs'] for lay in layers]))
    if not want_grads:
        return res
    p = np.exp(logits - lse[:, None])
    p[np.arange(R * T), yf] -= 1.0
    dlogits = p * W.reshape(-1, 1)
    g = dict(softmax_w=out.T.dot(dlogits), softmax_b=dlogits.sum(axis=0))
    dtop = dlogits.dot(params['softmax_w'].T).reshape(R, T, H)
    for l in reversed(range(L)):
        lay = layers[l]
        K = params['kernel_%d' % l]
        n_in = lay['x'].shape[2]
        if f is not None:
            dtop = dtop * f[l + 1].astype(dt)
        dz_all = np.zeros((R, T, 4 * H), dt)
        dh_rec, dc = np.zeros((R, H), dt), np.zeros((R, H), dt)
        for t in reversed(range(T)):
            si, tj, sf, so = lay['gates'][t]
            tc = np.tanh(lay['cs'][t + 1])
            dh = dtop[:, t] + dh_rec
            do = dh * tc * so * (1.0 - so)
            dc = dc + dh * so * (1.0 - tc * tc)
            dz = np.concatenate([dc * tj * si * (1.0 - si), dc * si * (1.0 - tj * tj), dc * lay['cs'][t] * sf * (1.0 - sf), do], axis=1)
            dz_all[:, t] = dz
            dh_rec = dz.dot(K[n_in:].T)
            dc = dc * sf                                  # (what reaches slot 0 -- dh_rec, dc -- is dropped: truncated BPTT)
        dzf = dz_all.reshape(R * T, 4 * H)
        hprev = np.transpose(lay['hs'][:-1], (1, 0, 2)).copy()
        if not dk_hprev:
            hprev[:, 0] = 0                               # planted: the t = 0 term multiplied by zeros, as with a zero state
        g['kernel_%d' % l] = np.concatenate([lay['x'].reshape(R * T, n_in).T.dot(dzf), hprev.reshape(R * T, H).T.dot(dzf)], axis=0)
        g['bias_%d' % l] = dzf.sum(axis=0)
        dtop = dzf.dot(K[:n_in].T).reshape(R, T, n_in)
    if f is not None:
        dtop = dtop * f[0].astype(dt)
    demb = np.zeros_like(params['embedding'])
    np.add.at(demb, (X if emb_rows is None else emb_rows).reshape(R * T), dtop.reshape(R * T, -1))
    g['embedding'] = demb
    res['grads'] = g
    res['aux'] = dict(embedding_slices_sq=float((dtop.astype(np.float64) ** 2).sum()))      # what the tf1_slices clip norm sees
    return res


def segment(params, state, tokens, lengths, cfg, dtype=np.float64, want_grads=True, mistake=None, prev=None, f=None):
    """One state pass -> (result, state').  result: loss (the masked mean NLL over n_valid), logprob [R, T] (0 behind a row's end), grads,
    n_valid, y [R, T] (the context tokens the call adds).  prev = (state before the previous segment, its tokens, its lengths): only
    the planted 'grad_through_state' reads it."""
    assert mistake is None or mistake in MISTAKES
    d = O.model_dims(cfg)
    start, T = d['start'], d['T']
    tokens = np.asarray(tokens, np.int64)
    R = tokens.shape[0]
    ln = np.full(R, T, np.int64) if lengths is None else np.asarray(lengths, np.int64)
    assert tokens.shape == (R, T) and ln.shape == (R,) and ln.min() >= 0 and ln.max() <= T and ln.sum() > 0
    p = {k: np.asarray(v, dtype) for k, v in params.items()}
    pending = np.full(R, start, np.int64) if mistake == 'start_word' else state['pending']
    X, Y, mask = device_xy(tokens, ln, pending, start)
    n_valid = int(ln.sum())
    W = np.where(mask, dtype(1.0 / (n_valid + 1e-12)), dtype(0.0))
    h0, c0 = np.asarray(state['h'], dtype), np.asarray(state['c'], dtype)
    if mistake == 'no_c':
        c0 = np.zeros_like(c0)
    if mistake == 'swap_layers':
        h0, c0 = h0[::-1], c0[::-1]
    emb_rows = None
    if mistake == 'table_start':
        emb_rows = X.copy()
        emb_rows[:, 0] = start
    if mistake == 'grad_through_state':
        # the gradient of THIS segment's loss through the previous segment as well: one pass over both, weights on this one only
        s0, tok0, ln0 = prev
        assert np.all(np.asarray(ln0) == T), 'a full previous segment: its end is the state'
        X0, Y0, _ = device_xy(tok0, ln0, s0['pending'], start)
        both = run(p, np.asarray(s0['h'], dtype), np.asarray(s0['c'], dtype), np.concatenate([X0, X], 1), np.concatenate([Y0, Y], 1),
                   np.concatenate([np.zeros_like(W), W], 1), cfg)
        r = run(p, h0, c0, X, Y, W, cfg, want_grads=False)
        r['grads'] = both['grads']
    else:
        r = run(p, h0, c0, X, Y, W, cfg, want_grads=want_grads, dk_hprev=mistake != 'no_hprev_dk', emb_rows=emb_rows, f=f)
    at = np.full(R, T, np.int64) if mistake == 'export_T' else ln
    rows = np.arange(R)
    h1 = np.where((at > 0)[None, :, None], r['hs'][:, at, rows], h0)
    c1 = np.where((at > 0)[None, :, None], r['cs'][:, at, rows], c0)
    last = np.where(ln > 0, tokens[rows, np.maximum(ln - 1, 0)], state['pending'])
    y = np.where(mask, tokens, last[:, None])
    out = dict(loss=r['loss'], logprob=np.where(mask, r['logprob'], 0), n_valid=n_valid, y=y, hs=r['hs'], cs=r['cs'], X=X, Y=Y)
    if 'grads' in r:
        out['grads'] = r['grads']
    if 'aux' in r:
        out['aux'] = r['aux']
    return out, dict(h=h1, c=c1, pending=last.astype(np.int64), ctx=np.concatenate([state['ctx'], y], axis=1))


def ragged_lengths(rng, R, T):
    """every kind of row: full, empty, one token, the rest random in [1, T]"""
    ln = rng.randint(1, T + 1, size=R)
    ln[0] = T
    if R > 1:
        ln[1] = 0
    if R > 2:
        ln[2] = 1
    return ln.astype(np.int32)


def segments(cfg, R, n, seed):
    """n consecutive segments [n][R, T] of random ids"""
    rng = np.random.RandomState(seed)
    return [rng.randint(0, cfg['input_size'], size=(R, cfg['max_len'])).astype(np.int32) for _ in range(n)]
