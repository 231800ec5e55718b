"""fp64 restatement of the padding-masked loss and its gradients (TEST INFRASTRUCTURE ONLY).

Built on oracle.lstm_oracle.forward's cache, which holds logits, lse and ce per position (row order b*T + t).  Row b has a length
len[b] in [1, T]; position t of row b is scored iff t < len[b]; n_valid = sum(len):

    loss = sum_{b, t < len[b]} ce[b][t] / (n_valid + 1e-12)
    dlogits[b][t] = (softmax - onehot) * mask[b][t] / (n_valid + 1e-12)

-- TF's sequence_loss with 0 / 1 weights, average_across_timesteps and average_across_batch both true.  The backward pass is
tests/backward_ref.py's / the oracle's arithmetic in the oracle's order; the division form is kept, so that with every length T the
loss and every gradient are the oracle's bit for bit.
"""
import numpy as np

from oracle import lstm_oracle as O


def mask_of(lengths, T):
    """lengths [B] -> float64 [B*T] in the oracle's row order b*T + t"""
    lengths = np.asarray(lengths).reshape(-1)
    assert lengths.min() >= 1 and lengths.max() <= T, lengths
    return (np.arange(T)[None, :] < lengths[:, None]).astype(np.float64).reshape(-1)


def masked_loss(cache, lengths, config):
    T = O.model_dims(config)['T']
    mask = mask_of(lengths, T)
    n_valid = int(np.asarray(lengths).sum())
    return (cache['ce'] * mask.astype(cache['ce'].dtype)).sum() / (n_valid + 1e-12)


def masked_backward(params, cache, config, lengths):
    """O.backward with dlogits = p * mask / (n_valid + 1e-12) -> (grads, aux)"""
    d = O.model_dims(config)
    H, L, T = d['H'], d['L'], d['T']
    B = cache['B']
    dtype = params['embedding'].dtype
    n = B * T
    grads = {}
    mask = mask_of(lengths, T).astype(dtype)
    n_valid = int(np.asarray(lengths).sum())

    p = np.exp(cache['logits'] - cache['lse'][:, None])
    p[np.arange(n), cache['Y'].reshape(n)] -= 1.0
    dlogits = p * mask[:, None] / dtype.type(n_valid + 1e-12)
    grads['softmax_w'] = cache['out'].T.dot(dlogits)
    grads['softmax_b'] = dlogits.sum(axis=0)
    dtop = dlogits.dot(params['softmax_w'].T).reshape(B, T, H)

    for l in reversed(range(L)):
        lay = cache['layers'][l]
        K = params['kernel_%d' % l]
        n_in = lay['x'].shape[2]
        Kh = K[n_in:]
        dz_all = np.zeros((B, T, 4 * H), dtype)
        dh_rec = np.zeros((B, H), dtype)
        dc = np.zeros((B, H), dtype)
        for t in reversed(range(T)):
            si, tj, sf, so = lay['gates'][t]
            c_t, c_prev = lay['cs'][t + 1], lay['cs'][t]
            tc = np.tanh(c_t)
            dh = dtop[:, t] + dh_rec
            do = dh * tc * so * (1.0 - so)
            dc = dc + dh * so * (1.0 - tc * tc)
            di = dc * tj * si * (1.0 - si)
            dj = dc * si * (1.0 - tj * tj)
            df = dc * c_prev * sf * (1.0 - sf)
            dz = np.concatenate([di, dj, df, do], axis=1)
            dz_all[:, t] = dz
            dh_rec = dz.dot(Kh.T)
            dc = dc * sf
        dzf = dz_all.reshape(n, 4 * H)
        hprev = np.transpose(lay['hs'][:-1], (1, 0, 2)).reshape(n, H)
        xin = lay['x'].reshape(n, n_in)
        grads['kernel_%d' % l] = np.concatenate([xin.T.dot(dzf), hprev.T.dot(dzf)], axis=0)
        grads['bias_%d' % l] = dzf.sum(axis=0)
        dtop = dzf.dot(K[:n_in].T).reshape(B, T, n_in)

    dx = dtop.reshape(n, -1)
    demb = np.zeros_like(params['embedding'])
    np.add.at(demb, cache['X'].reshape(n), dx)
    grads['embedding'] = demb
    aux = dict(embedding_slices_sq=float((dx.astype(np.float64) ** 2).sum()))
    return grads, aux


def device_xy(sup, qry, support_len, query_len, cfg):
    """-> X, Y [B, T] as the device's masked pass sees them: O.train_xy, then what token_prep_body<true> does (elementwise.hip
    k_token_prep_len: `if (t >= l) tok_y = 0; if (t + 1 >= l) tok = start_word;`) -- at t >= len[b] the input id is
    the start word and the target is 0, whatever the caller put behind the song's end.  A reference built from these has the
    device's hs, cs, logits, lse and ce on ALL rows, the masked ones included: ce and lse stay per-row values on a masked pass
    (elementwise.hip: ce_rows_body `ce[r] = l - row[t]`, ce_row_reg `ce[r] = l - xt`, ce_finish_body `ce[row] = l - logf(et)`, each
    before the row's weight is used at all; k_loss_reduce_w `if (w[r] != 0.0f) s += (double)ce[r];` adds the unweighted values and
    divides once by n_valid), only dlogits carries the weight."""
    X, Y = O.train_xy(sup, qry, cfg['input_size'])
    ln = train_lengths(support_len, query_len)
    pad = np.arange(X.shape[1])[None, :] >= ln[:, None]
    X, Y = X.copy(), Y.copy()
    X[pad] = cfg['input_size']                 # the start word (O.train_xy's third argument)
    Y[pad] = 0
    return X, Y


def train_lengths(support_len, query_len):
    """[N,K] + [N,Q] -> [N*K + N*Q], support rows first (the order of O.train_xy)"""
    return np.concatenate([np.asarray(support_len).reshape(-1), np.asarray(query_len).reshape(-1)])


def step(params, sup, qry, support_len, query_len, config):
    """one masked forward + backward -> (loss, cache, grads, aux)"""
    X, Y = O.train_xy(sup, qry, config['input_size'])
    _, cache = O.forward(params, X, Y, config)
    lengths = train_lengths(support_len, query_len)
    grads, aux = masked_backward(params, cache, config, lengths)
    return float(masked_loss(cache, lengths, config)), cache, grads, aux


def train_step(params, opt, sup, qry, support_len, query_len, config):
    """O.train_step with the masked loss: the loss at the pre-update parameters, then one clip + Adam update (in place)"""
    loss, _, grads, aux = step(params, sup, qry, support_len, query_len, config)
    O.apply_update(params, grads, aux, opt, config)
    return loss


def eval_step(params, qry, query_len, config):
    X, Y = O.eval_xy(qry, config['input_size'])
    _, cache = O.forward(params, X, Y, config)
    return float(masked_loss(cache, np.asarray(query_len).reshape(-1), config))


def lengths_for(rng, shape, T):
    """seeded lengths that always hold a 1, a T and values in between"""
    n = int(np.prod(shape))
    ln = rng.randint(1, T + 1, size=n)
    idx = rng.permutation(n)
    ln[idx[0]] = T
    if n >= 2:
        ln[idx[1]] = 1
    if n >= 3 and T >= 3:
        ln[idx[2]] = T // 2 + 1
    return ln.reshape(shape).astype(np.int32)


def scramble_padding(tokens, lengths, vocab, rng):
    """a copy of tokens [..., T] with every position t >= len replaced by another in-range id"""
    tokens = np.asarray(tokens)
    T = tokens.shape[-1]
    pad = np.arange(T) >= np.asarray(lengths)[..., None]
    out = tokens.copy()
    out[pad] = rng.randint(0, vocab, size=int(pad.sum()))
    return out.astype(tokens.dtype)


def componentwise_lengths(cfg, N, K, Q, seed):
    """-> (support_len [N,K], query_len [N,Q]) of the element-by-element masked tests, for a shape of backward_ref.CW_SHAPES: the
    seeded lengths_for, then forced so that the edges exist whatever the seed gives:
      * with B >= 32 rows, rows b = 16 .. 31 of the pass's row order (support rows first) get a length <= T // 2: in the late steps
        one whole 16-row tile of the recurrence is masked while its neighbours are mixed;
      * a 1, a T and (B >= 3, T >= 3) a value strictly between, at rows outside that tile."""
    T, B = cfg['max_len'], N * (K + Q)
    rng = np.random.RandomState(1000 + seed)
    ln = lengths_for(rng, (B,), T)
    free = np.arange(B)
    if B >= 32:
        ln[16:32] = np.minimum(ln[16:32], T // 2)
        free = np.concatenate([free[:16], free[32:]])
    idx = free[rng.permutation(free.size)]
    ln[idx[0]] = T
    if B >= 2:
        ln[idx[1]] = 1
    if B >= 3 and T >= 3:
        ln[idx[2]] = T // 2 + 1
    return ln[:N * K].reshape(N, K).astype(np.int32), ln[N * K:].reshape(N, Q).astype(np.int32)
