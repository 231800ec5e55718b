"""Dynamic evaluation (include/fsmg.h "dynamic evaluation") restated in numpy (TEST INFRASTRUCTURE ONLY).

Built on oracle.lstm_oracle.forward's cache (logits, lse, ce per position, row order b * T + t) and on tests/masked_ref.py's backward
pass generalised from the mask t < len[b] to a window mask lo <= t < min(hi, len[b]).  `stream` walks a stream exactly as the header
states it -- blocks, windows, score before update, the two rules -- in the dtype of the parameters it is given: fp64 is the reference,
fp32 the yardstick e32 of the GPU tests (the same restatement on the same inputs, one precision down).

wrong= plants one mistake (WRONG); tests/test_dyneval_cpu.py shows that each one moves a reported log-prob or theta_l by more than the
GPU tests' bounds at the shapes they run, i.e. that those tests can tell.
"""
import numpy as np

from oracle import lstm_oracle as O

SGD, RMS = 0, 1
WRONG = ('score_after', 'decay_prev', 'mean_rms_pads', 'hi_plus_one', 'nvalid_row', 'no_cap')


def dyn_config(rule=SGD, seg_len=1, rows_per_step=1, lr=0.1, decay=0.0, eps=1e-3, clip_norm=0.0, adapt_reported=1):
    """the fields of fsmg_dyneval_config; the floats as the fp32 values the struct holds"""
    f = lambda v: float(np.float32(v))
    return dict(rule=int(rule), seg_len=int(seg_len), rows_per_step=int(rows_per_step), lr=f(lr), decay=f(decay), eps=f(eps),
                clip_norm=f(clip_norm), adapt_reported=int(adapt_reported))


def blocks_of(n_rows, first_reported, rows_per_step):
    """[(r0, r1, reported)]: boundaries at every multiple of rows_per_step, at first_reported and at n_rows"""
    out, r0 = [], 0
    while r0 < n_rows:
        r1 = min(n_rows, (r0 // rows_per_step + 1) * rows_per_step)
        if r0 < first_reported < r1:
            r1 = first_reported
        out.append((r0, r1, r0 >= first_reported))
        r0 = r1
    return out


def windows_of(T, S):
    return [(lo, min(lo + S, T)) for lo in range(0, T, S)]


def window_mask(lengths, T, lo, hi):
    """-> (mask float64 [B * T] in the oracle's row order, n_valid)"""
    e = np.minimum(np.asarray(lengths).reshape(-1), hi)
    t = np.arange(T)[None, :]
    m = (t >= lo) & (t < e[:, None])
    return m.astype(np.float64).reshape(-1), int(m.sum())


def weighted_backward(params, cache, config, mask, n_valid):
    """masked_ref.masked_backward with the mask and the divisor given: dlogits = (softmax - onehot) * mask / (n_valid + 1e-12)"""
    d = O.model_dims(config)
    H, L, T = d['H'], d['L'], d['T']
    B = cache['B']
    dtype = params['embedding'].dtype
    n = B * T
    grads = {}
    mask = np.asarray(mask).astype(dtype)
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
    return grads, dict(embedding_slices_sq=float((dx.astype(np.float64) ** 2).sum()))


def window_pass(params, rows, lengths, config, lo, hi, wrong=None):
    """one window pass over rows [B, T] -> (ce [B, T], mask [B, T] bool, n_valid, grads, aux, loss)"""
    T = O.model_dims(config)['T']
    X, Y = O.tokens_to_input_and_target(np.asarray(rows)[None], config['input_size'])
    _, cache = O.forward(params, X, Y, config)
    mask, n_valid = window_mask(lengths, T, lo, min(hi + 1, T) if wrong == 'hi_plus_one' else hi)
    if wrong == 'nvalid_row':
        n_valid = int(np.asarray(lengths).sum())
    grads, aux = weighted_backward(params, cache, config, mask, n_valid)
    B = X.shape[0]
    loss = float((cache['ce'].astype(np.float64) * mask).sum() / (n_valid + 1e-12))
    return cache['ce'].reshape(B, T), mask.reshape(B, T) > 0, n_valid, grads, aux, loss


def padded_elements(config):
    """the flat buffer's element count with its pads, near enough for the planted mistake that counts them (api_layout.hip: embedding
    and hidden widths to 16, the vocabulary to 4, every tensor to 64 floats)"""
    d = O.model_dims(config)
    up = lambda n, a: (n + a - 1) // a * a
    Ep, Hp, V1p = up(d['E'], 16), up(d['H'], 16), up(d['V1'], 4)
    n = up(d['V1'] * Ep, 64)
    for l in range(d['L']):
        n += up(((Ep if l == 0 else Hp) + Hp) * 4 * Hp, 64) + up(4 * Hp, 64)
    return n + up(Hp * V1p, 64) + up(V1p, 64)


def mean_rms_of(stats, config=None, wrong=None):
    """mean of sqrt(ms_sum / count) over the logical elements, fp64"""
    s = sum(float(np.sqrt(np.asarray(v, np.float64) / stats['count']).sum()) for v in stats['ms_sum'].values())
    n = sum(int(np.asarray(v).size) for v in stats['ms_sum'].values())
    if wrong == 'mean_rms_pads':
        n = padded_elements(config)
    return s / n


def update(theta_l, theta_g, grads, aux, dcfg, mode, stats=None, mean_rms=None, wrong=None, anchor=None):
    """one update in theta_l's dtype -> (new theta_l, gnorm, c)"""
    dt = theta_l['embedding'].dtype.type
    gnorm = float(O.global_norm(grads, aux, mode))
    clip = dcfg['clip_norm']
    c = clip / max(gnorm, clip) if clip > 0 else 1.0
    step = dt(dt(c) * dt(dcfg['lr']))
    decay = dt(dcfg['decay'])
    anchor = theta_g if anchor is None else anchor
    new = {}
    for k in theta_l:
        p, g = theta_l[k], grads[k].astype(theta_l[k].dtype)
        if dcfg['rule'] == RMS:
            r = np.sqrt(np.asarray(stats['ms_sum'][k]).astype(p.dtype) / dt(stats['count']))
            q = p - (step * g) / (r + dt(dcfg['eps']))
            if dcfg['decay'] != 0:
                ratio = r / dt(mean_rms)
                if wrong != 'no_cap':
                    ratio = np.minimum(dt(1.0) / decay, ratio)
                q = q + (decay * (anchor[k] - p)) * ratio
        else:
            q = p - step * g
            if dcfg['decay'] != 0:
                q = q + decay * (anchor[k] - p)
        new[k] = q
    return new, gnorm, c


def stream(params, tokens, lengths, config, dcfg, first_reported, stats=None, mode='tf1_slices', wrong=None):
    """the whole call, in the dtype of `params` -> dict(logprob [R, T] float64 (0 where nothing is reported), row_nll [R], nll, theta_l,
    updates = [dict(block, window, n_valid, gnorm, c, loss)], passes = the number of window passes)"""
    assert wrong is None or wrong in WRONG, wrong
    T = O.model_dims(config)['T']
    tokens = np.asarray(tokens)
    R = tokens.shape[0]
    lengths = np.full(R, T, np.int64) if lengths is None else np.asarray(lengths).reshape(-1)
    theta_g = {k: v.copy() for k, v in params.items()}
    theta_l = {k: v.copy() for k, v in params.items()}
    prev = theta_g
    mean_rms = mean_rms_of(stats, config, wrong) if dcfg['rule'] == RMS else None
    logprob = np.zeros((R, T), np.float64)
    updates, passes = [], 0
    for r0, r1, reported in blocks_of(R, first_reported, dcfg['rows_per_step']):
        adapt = (not reported) or dcfg['adapt_reported']
        for lo, hi in windows_of(T, dcfg['seg_len'] if adapt else T):
            mask, n_valid = window_mask(lengths[r0:r1], T, lo, hi)
            if n_valid == 0:
                continue
            ce, m, nv, grads, aux, loss = window_pass(theta_l, tokens[r0:r1], lengths[r0:r1], config, lo, hi, wrong)
            passes += 1
            true_m = mask.reshape(r1 - r0, T) > 0
            if reported and wrong != 'score_after':
                logprob[r0:r1][true_m] = -ce[true_m]
            if adapt:
                before = theta_l
                theta_l, gnorm, c = update(theta_l, theta_g, grads, aux, dcfg, mode, stats, mean_rms, wrong,
                                           anchor=prev if wrong == 'decay_prev' else None)
                prev = before
                updates.append(dict(block=(r0, r1), window=(lo, hi), n_valid=nv, gnorm=gnorm, c=c, loss=loss))
            if reported and wrong == 'score_after':
                ce2 = window_pass(theta_l, tokens[r0:r1], lengths[r0:r1], config, lo, hi)[0]
                logprob[r0:r1][true_m] = -ce2[true_m]
    row_nll = np.zeros(R, np.float32)
    total, count = 0.0, 0
    for r in range(first_reported, R):
        s = 0.0
        for t in range(int(lengths[r])):
            s += float(np.float32(logprob[r, t]))
            total += float(np.float32(logprob[r, t]))
        row_nll[r] = np.float32(-s)
        count += int(lengths[r])
    return dict(logprob=logprob, row_nll=row_nll, nll=(-total / count if count else float('nan')), theta_l=theta_l, updates=updates,
                passes=passes, count=count)


def host_nll(logprob32, lengths, first_reported):
    """the library's host arithmetic on the fp32 array it returned: (row_nll float32 [R], nll float32) -- fp64 sums in (row, position)
    order, each rounded once"""
    R, T = logprob32.shape
    lengths = np.full(R, T, np.int64) if lengths is None else np.asarray(lengths).reshape(-1)
    row = np.zeros(R, np.float32)
    total, count = 0.0, 0
    for r in range(first_reported, R):
        s = 0.0
        for t in range(int(lengths[r])):
            s += float(logprob32[r, t])
            total += float(logprob32[r, t])
        row[r] = np.float32(-s)
        count += int(lengths[r])
    return row, (np.float32(-total / count) if count else np.float32('nan'))


def update_check(label, theta_prev, theta_g, grads, tail, mode, dcfg, stats, mean_rms, got_theta, got_gnorm, verbose=True):
    """k_dyneval_update (dyneval.hip) redone in fp64 from what a device holds, all fp32: the previous theta_l, theta_g, the gradient,
    its tail, ms_sum, count and the mean_rms the device computed.  The kernel's roundings, element by element (u = 2^-24):
        step = fl(fl(clip / max(gnorm, clip)) * lr)                           3 roundings incl. the norm it came from
        SGD:  t1 = fl(step * g);  q = fl(p - t1);  t2 = fl(decay * fl(pg - p));  out = fl(q + t2)
        RMS:  r = fl(sqrt(fl(ms / cnt)));  t1 = fl(fl(step * g) / fl(r + eps));  t2 = fl(fl(decay * fl(pg - p)) * min(1 / decay, fl(r / mean_rms)))
    so, with the terms evaluated exactly in fp64 from the fp32 inputs,
        |got - ref| <= 2 u |ref| + 2 u |p - t1| + 8 u |t1| + 6 u |t2| + 1e-30
    -- t1 carries the step's three roundings plus its own product, (RMS) the quotient, the root, the inner quotient and the sum with
    eps, each at most 1 u of t1: 8 u covers them; t2 the difference, the product, (RMS) the ratio, the reciprocal of decay and the last
    product: 6 u; the two sums one rounding each of their results.  Derived from the operation count, not from a run.
    An element with g == 0 and pg == p must keep p's bits.  -> failures (list of strings)"""
    import maml_ref as M
    U = M.U
    gnorm = M.device_gnorm(grads, tail, mode)
    failures = []
    if not abs(float(got_gnorm) - gnorm) <= 2 * U * gnorm:
        failures.append('gnorm %.9g, from the gradients %.9g' % (float(got_gnorm), gnorm))
    clip = dcfg['clip_norm']
    c = float(np.float32(clip / max(gnorm, clip))) if clip > 0 else 1.0
    step = float(np.float32(np.float32(c) * np.float32(dcfg['lr'])))
    decay = dcfg['decay']
    for k in sorted(grads):
        p, g, pg, got = (np.asarray(a) for a in (theta_prev[k], grads[k], theta_g[k], got_theta[k]))
        assert p.dtype == g.dtype == pg.dtype == got.dtype == np.float32, k
        p64, g64, pg64 = p.astype(np.float64), g.astype(np.float64), pg.astype(np.float64)
        t1 = step * g64
        t2 = np.zeros_like(p64)
        if dcfg['rule'] == RMS:
            r = np.sqrt(np.asarray(stats['ms_sum'][k], np.float64) / float(stats['count']))
            t1 = t1 / (r + dcfg['eps'])
            if decay != 0:
                t2 = decay * (pg64 - p64) * np.minimum(float(np.float32(1.0) / np.float32(decay)), r / float(mean_rms))
        elif decay != 0:
            t2 = decay * (pg64 - p64)
        ref = (p64 - t1) + t2
        tol = 2 * U * np.abs(ref) + 2 * U * np.abs(p64 - t1) + 8 * U * np.abs(t1) + 6 * U * np.abs(t2) + 1e-30
        frac = np.abs(got.astype(np.float64) - ref) / tol
        still = (g == 0) & (pg.view(np.uint32) == p.view(np.uint32)) & (got.view(np.uint32) != p.view(np.uint32))
        if verbose:
            print('DYNUPD|%s|%s|%.3f' % (label, k, frac.max()))
        if not np.all(np.isfinite(got)) or (frac > 1).any():
            failures.append('%s: %d of %d outside the bound (worst %.2f x)' % (k, int((frac > 1).sum()), frac.size, frac.max()))
        if still.any():
            failures.append('%s: %d elements with nothing to move them moved' % (k, int(still.sum())))
    return failures
