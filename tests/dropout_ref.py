"""Dropout of the train passes, restated on the host (TEST INFRASTRUCTURE ONLY; include/fsmg.h "Dropout").

  * philox4x32_10: the counter-based generator in numpy (Salmon et al. 2011, the Random123 constants), held to three known answers
    by tests/test_dropout_cpu.py; site_mask / factors rebuild every mask of a pass from (seed, pass, site, row, unit) -- nothing
    here ever asks the device for a mask;
  * forward_drop / backward_drop: oracle.lstm_oracle.forward and backward_ref.backward_full with the factors mask * scale at the
    sites.  The added multiplications are by exactly 1.0 where a keep is 1, so with all keeps 1 both are the undropped functions
    bit for bit;
  * DropReference: backward_ref.Reference for a dropped pass -- the fp64 pass, its fp32 restatement with the same factors, e32 per
    family in the family's own measure, plus the family 'drop' (the masked activations of every site, one (t, b) row per slice);
  * the `mistake` arguments plant the errors tests/test_dropout_cpu.py shows its assertions to catch.

The scale is the device's: 1.0f / keep in fp32, ONE value, taken as it is by the fp64 pass too (the semantics fix it; an fp64
quotient would be another model).
"""
import numpy as np

import backward_ref as R
from oracle import lstm_oracle as O

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
GOLDEN64 = 0x9E3779B97F4A7C15         # fsmg/dist.py: rank r trains with seed + r * GOLDEN64 mod 2^64

MISTAKES = ('bwd_no_scale', 'variational_t', 'recurrent_masked', 'sites_swapped', 'eval_dropped', 'thr_round')


# ----------------------------------------------------------------------------- the generator
def philox4x32_10(counter, key):
    """counter: uint32 [..., 4], key: (k0, k1) -> uint32 [..., 4]"""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c[0], PHILOX_M1 * c[2]                  # 32 x 32 -> 64 bits: no overflow in uint64
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & M32, p1 & M32, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & M32, p0 & M32]
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return np.stack(c, axis=-1).astype(np.uint32)


def threshold(keep, mistake=None):
    """thr = (uint32)(keep_f32 * 16777216.0f): truncation"""
    v = np.float32(keep) * np.float32(16777216.0)
    return int(np.rint(v)) if mistake == 'thr_round' else int(v)


def scale_of(keep):
    """1.0f / keep_f32, one fp32 rounding"""
    return np.float32(1.0) / np.float32(keep)


def kept(words, keep, mistake=None):
    """the decision on the generator's words: kept iff (word >> 8) < thr"""
    return (np.asarray(words, np.uint32) >> np.uint32(8)) < np.uint32(threshold(keep, mistake))


def site_mask(seed, pass_index, site, T, B, W, keep, variational, mistake=None):
    """-> uint8 [T, B, W], the device's row order t * B + b: 1 where the element is kept"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    t, b, j4 = np.meshgrid(np.arange(T, dtype=np.int64), np.arange(B, dtype=np.int64), np.arange((W + 3) // 4, dtype=np.int64), indexing='ij')
    row = b if (variational and mistake != 'variational_t') else t * B + b
    ctr = np.stack([j4, row, np.full_like(j4, site), np.full_like(j4, int(pass_index) & 0xFFFFFFFF)], axis=-1).astype(np.uint32)
    words = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).reshape(T, B, -1)[:, :, :W]      # element j: word j & 3 of call j >> 2
    return kept(words, keep, mistake).astype(np.uint8)


def keep_of(drop, site):
    return drop.get('keep_input', 1.0) if site == 0 else drop.get('keep_output', 1.0)


def factors(config, drop, pass_index, B, dtype=np.float64, mistake=None):
    """-> [L + 1] arrays [B, T, W] (the oracle's order) of mask * scale for the pass; drop: dict(keep_input, keep_output,
    variational, seed).  A site whose keep is 1 is all ones."""
    d = O.model_dims(config)
    out = []
    for site in range(d['L'] + 1):
        W = d['E'] if site == 0 else d['H']
        keep = keep_of(drop, site)
        if float(np.float32(keep)) == 1.0:
            out.append(np.ones((B, d['T'], W), dtype))
            continue
        m = site_mask(drop.get('seed', 0), pass_index, site, d['T'], B, W, keep, drop.get('variational', False), mistake)
        out.append(np.transpose(m, (1, 0, 2)).astype(dtype) * dtype(scale_of(keep)))
    if mistake == 'sites_swapped':
        assert d['L'] >= 2
        out[1], out[2] = out[2], out[1]
    return out


def ones(config, B, dtype=np.float64):
    d = O.model_dims(config)
    return [np.ones((B, d['T'], d['E'] if s == 0 else d['H']), dtype) for s in range(d['L'] + 1)]


# ----------------------------------------------------------------------------- the dropped pass
def forward_drop(params, X, Y, config, f, mistake=None):
    """oracle.lstm_oracle.forward with the factors f[site] at the sites -> (loss, cache); cache['layers'][l]['x'] is the MASKED
    input of layer l, cache['out'] the masked top output, hs / cs the unmasked states, cache['drop'][site] the masked activations"""
    d = O.model_dims(config)
    H, L, T = d['H'], d['L'], d['T']
    dtype = params['embedding'].dtype
    X, Y = np.asarray(X), np.asarray(Y)
    B = X.shape[0]
    assert X.shape == (B, T) and Y.shape == (B, T)
    drop = []
    layer_in = params['embedding'][X] * f[0].astype(dtype)
    drop.append(layer_in)
    layers = []
    for l in range(L):
        K, b = params['kernel_%d' % l], params['bias_%d' % l]
        n_in = layer_in.shape[2]
        Kx, Kh = K[:n_in], K[n_in:]
        zx = layer_in.reshape(B * T, n_in).dot(Kx).reshape(B, T, 4 * H) + b
        h = np.zeros((B, H), dtype)
        c = np.zeros((B, H), dtype)
        hs = np.zeros((T + 1, B, H), dtype)
        cs = np.zeros((T + 1, B, H), dtype)
        gates = np.zeros((T, 4, B, H), dtype)
        for t in range(T):
            z = zx[:, t] + h.dot(Kh)
            i, j, fg, o = z[:, :H], z[:, H:2 * H], z[:, 2 * H:3 * H], z[:, 3 * H:]
            si, tj, sf, so = O._sigmoid(i), np.tanh(j), O._sigmoid(fg + O.FORGET_BIAS), O._sigmoid(o)
            c = c * sf + si * tj
            h = np.tanh(c) * so
            hs[t + 1], cs[t + 1] = h, c
            gates[t, 0], gates[t, 1], gates[t, 2], gates[t, 3] = si, tj, sf, so
            if mistake == 'recurrent_masked':
                h = h * f[l + 1][:, t].astype(dtype)
        layers.append(dict(x=layer_in, hs=hs, cs=cs, gates=gates))
        layer_in = np.transpose(hs[1:], (1, 0, 2)) * f[l + 1].astype(dtype)
        drop.append(layer_in)
    out = layer_in.reshape(B * T, H)
    logits = out.dot(params['softmax_w']) + params['softmax_b']
    m = logits.max(axis=1)
    lse = m + np.log(np.exp(logits - m[:, None]).sum(axis=1))
    yflat = Y.reshape(B * T)
    ce = lse - logits[np.arange(B * T), yflat]
    loss = ce.sum() / (B * T + 1e-12)
    return dtype.type(loss), dict(X=X, Y=Y, layers=layers, out=out, logits=logits, lse=lse, ce=ce, B=B, drop=drop)


def backward_drop(params, cache, config, f, weights=None, mistake=None):
    """backward_ref.backward_full with the factors on the gradient that flows back through every site; same returns.  dh is what
    arrives at layer 0's chain (masked by site 1), dx the masked embedding slices; a dropped position has S == 0 there."""
    if mistake == 'bwd_no_scale':
        f = [(a != 0).astype(a.dtype) for a in f]
    d = O.model_dims(config)
    H, L, T = d['H'], d['L'], d['T']
    B = cache['B']
    dtype = params['embedding'].dtype
    n = B * T
    grads, scales = {}, {}
    yflat = cache['Y'].reshape(n)
    p = np.exp(cache['logits'] - cache['lse'][:, None])
    s_dlogits = p.copy()
    s_dlogits[np.arange(n), yflat] += 1.0
    p[np.arange(n), yflat] -= 1.0
    if weights is None:
        scales['dlogits'] = s_dlogits / dtype.type(n + 1e-12)
        dlogits = p / dtype.type(n + 1e-12)
    else:
        mask = np.asarray(weights).reshape(n).astype(dtype)
        n_valid = int(mask.sum())
        scales['dlogits'] = s_dlogits * mask[:, None] / dtype.type(n_valid + 1e-12)
        dlogits = p * mask[:, None] / dtype.type(n_valid + 1e-12)
    a_dl = np.abs(dlogits)
    grads['softmax_w'] = cache['out'].T.dot(dlogits)
    grads['softmax_b'] = dlogits.sum(axis=0)
    scales['softmax_w'] = np.abs(cache['out']).T.dot(a_dl)
    scales['softmax_b'] = a_dl.sum(axis=0)
    fa = [np.abs(a).astype(dtype) for a in f]
    dtop = dlogits.dot(params['softmax_w'].T).reshape(B, T, H) * f[L].astype(dtype)
    s_dtop = a_dl.dot(np.abs(params['softmax_w']).T) * fa[L].reshape(n, H)
    a_out = np.abs(cache['out'])
    scales['logits'] = a_out.dot(np.abs(params['softmax_w'])) + np.abs(params['softmax_b'])
    scales['lse'] = np.abs(cache['lse'])
    scales['ce'] = np.abs(cache['lse']) + np.abs(cache['logits'][np.arange(n), yflat])
    dz_layers = [None] * L
    dh = s_dh = None
    for l in reversed(range(L)):
        lay = cache['layers'][l]
        K = params['kernel_%d' % l]
        n_in = lay['x'].shape[2]
        Kh = K[n_in:]
        if l == 0:
            dh, s_dh = dtop.reshape(n, H), s_dtop
        dz_all = np.zeros((B, T, 4 * H), dtype)
        dh_rec = np.zeros((B, H), dtype)
        dc = np.zeros((B, H), dtype)
        for t in reversed(range(T)):
            si, tj, sf, so = lay['gates'][t]
            c_t, c_prev = lay['cs'][t + 1], lay['cs'][t]
            tc = np.tanh(c_t)
            dht = dtop[:, t] + dh_rec
            do = dht * tc * so * (1.0 - so)
            dc = dc + dht * so * (1.0 - tc * tc)
            di = dc * tj * si * (1.0 - si)
            dj = dc * si * (1.0 - tj * tj)
            df = dc * c_prev * sf * (1.0 - sf)
            dz = np.concatenate([di, dj, df, do], axis=1)
            dz_all[:, t] = dz
            dh_rec = dz.dot(Kh.T)
            dc = dc * sf
        dzf = dz_all.reshape(n, 4 * H)
        dz_layers[l] = dzf
        a_dz = np.abs(dzf)
        hprev = np.transpose(lay['hs'][:-1], (1, 0, 2)).reshape(n, H)
        xin = lay['x'].reshape(n, n_in)
        grads['kernel_%d' % l] = np.concatenate([xin.T.dot(dzf), hprev.T.dot(dzf)], axis=0)
        grads['bias_%d' % l] = dzf.sum(axis=0)
        scales['kernel_%d' % l] = np.concatenate([np.abs(xin).T.dot(a_dz), np.abs(hprev).T.dot(a_dz)], axis=0)
        scales['bias_%d' % l] = a_dz.sum(axis=0)
        dtop = dzf.dot(K[:n_in].T).reshape(B, T, n_in) * f[l].astype(dtype)
        s_dtop = a_dz.dot(np.abs(K[:n_in]).T) * fa[l].reshape(n, n_in)
    dx = dtop.reshape(n, -1)
    demb = np.zeros_like(params['embedding'])
    np.add.at(demb, cache['X'].reshape(n), dx)
    grads['embedding'] = demb
    s_emb = np.zeros_like(params['embedding'])
    np.add.at(s_emb, cache['X'].reshape(n), s_dtop)
    scales['embedding'] = s_emb
    scales['dx'] = s_dtop
    scales['dh'] = s_dh
    aux = dict(embedding_slices_sq=float((dx.astype(np.float64) ** 2).sum()))
    return dict(grads=grads, aux=aux, dlogits=dlogits, dz=dz_layers, dx=dx, dh=dh, scales=scales)


def eval_drop(params, query, config, drop=None, mistake=None):
    """evaluation never drops: oracle.lstm_oracle.eval_step -- unless the mistake is planted"""
    X, Y = O.eval_xy(query, O.model_dims(config)['start'])
    f = factors(config, drop, 0, X.shape[0]) if mistake == 'eval_dropped' else ones(config, X.shape[0])
    return float(forward_drop(params, X, Y, config, f)[0])


def train_step_drop(params, opt, support, query, config, drop, pass_index, clip_norm_mode='tf1_slices', weights=None):
    """oracle.lstm_oracle.train_step as a dropped pass with index pass_index; mutates params / opt -> the loss"""
    X, Y = O.train_xy(support, query, O.model_dims(config)['start'])
    f = factors(config, drop, pass_index, X.shape[0], params['embedding'].dtype.type)
    loss, cache = forward_drop(params, X, Y, config, f)
    full = backward_drop(params, cache, config, f, weights)
    O.apply_update(params, full['grads'], full['aux'], opt, config, clip_norm_mode)
    return float(loss)


def maml_step_drop(params, opt, support, query, config, drop, first_pass, inner_steps=1, inner_lr=0.1, clip_norm_mode='tf1_slices'):
    """oracle.lstm_oracle.maml_step with dropped passes first_pass .. first_pass + inner_steps (the query pass takes the last);
    mutates params / opt -> the query loss at theta'"""
    d = O.model_dims(config)
    dt = params['embedding'].dtype.type
    fast = {k: v.copy() for k, v in params.items()}
    X, Y = O.tokens_to_input_and_target(support, d['start'])
    clip = float(config['max_grad_norm'])
    for i in range(int(inner_steps)):
        f = factors(config, drop, first_pass + i, X.shape[0], dt)
        _, cache = forward_drop(fast, X, Y, config, f)
        full = backward_drop(fast, cache, config, f)
        scale = clip / max(O.global_norm(full['grads'], full['aux'], clip_norm_mode), clip)
        for k in fast:
            fast[k] = fast[k] - dt(inner_lr) * (full['grads'][k] * dt(scale))
    Xq, Yq = O.tokens_to_input_and_target(query, d['start'])
    f = factors(config, drop, first_pass + int(inner_steps), Xq.shape[0], dt)
    loss, cache = forward_drop(fast, Xq, Yq, config, f)
    full = backward_drop(fast, cache, config, f)
    O.apply_update(params, full['grads'], full['aux'], opt, config, clip_norm_mode)
    return float(loss)


# ----------------------------------------------------------------------------- the reference of one dropped pass
FAMILIES = R.FAMILIES + ('drop',)
SLICE_AXES = dict(R.SLICE_AXES, drop=(2,))            # one (b, t) row of a site's units


def _tensors(params, X, Y, config, f, weights=None):
    dtype = params['embedding'].dtype
    f = [a.astype(dtype) for a in f]
    loss, cache = forward_drop(params, X, Y, config, f)
    full = backward_drop(params, cache, config, f, weights)
    if weights is not None:                            # the padding-masked loss (masked_ref.masked_loss)
        mask = np.asarray(weights).reshape(-1)
        loss = (cache['ce'] * mask.astype(cache['ce'].dtype)).sum() / (int(mask.sum()) + 1e-12)
    B = cache['B']
    H, T = config['hidden_size'], config['max_len']
    t = {('logits', None): cache['logits'], ('lse', None): cache['lse'], ('ce', None): cache['ce'],
         ('dlogits', None): full['dlogits'], ('dh', None): full['dh'], ('dx', None): full['dx'],
         ('softmax_w', None): full['grads']['softmax_w'], ('softmax_b', None): full['grads']['softmax_b'],
         ('embedding', None): full['grads']['embedding']}
    for l in range(config['n_layers']):
        t[('kernel', l)] = full['grads']['kernel_%d' % l]
        t[('bias', l)] = full['grads']['bias_%d' % l]
        t[('hs', l)] = cache['layers'][l]['hs']
        t[('cs', l)] = cache['layers'][l]['cs']
        t[('dz', l)] = full['dz'][l].reshape(B, T, 4, H)
    for s, a in enumerate(cache['drop']):
        t[('drop', s)] = a                                                             # [B, T, W]
    return float(loss), cache, full, t


class DropReference(object):
    """backward_ref.Reference for one dropped pass: f = factors(...) of the pass, weights as backward_full's"""

    def __init__(self, params64, X, Y, config, f, weights=None):
        self.config, self.params, self.f = config, params64, f
        self.loss, self.cache, self.full, self.t = _tensors(params64, X, Y, config, f, weights)
        p32 = {k: v.astype(np.float32) for k, v in params64.items()}
        _, _, _, t32 = _tensors(p32, X, Y, config, f, weights)
        self.e32 = {}
        for (fam, layer), a32 in t32.items():
            assert a32.dtype == np.float32, (fam, a32.dtype)
            if fam in R.COMPONENTWISE:
                assert np.all(a32[R.scale_of(self.full, fam, layer) == 0] == 0), fam
            self.e32[fam] = max(self.e32.get(fam, 0.0), float(self.measure(fam, layer, a32).max()))

    def measure(self, fam, layer, got):
        ref = self.t[(fam, layer)]
        if fam in SLICE_AXES:
            return R.slice_ratio(got, ref, SLICE_AXES[fam])
        return R.componentwise_ratio(got, ref, R.scale_of(self.full, fam, layer))

    def ratio(self, fam, layer, got):
        m = self.measure(fam, layer, got)
        i = np.unravel_index(int(np.argmax(m)), m.shape)
        return float(m[i]) / max(self.e32[fam], 1e-300), i

    def failures(self, fam, layer, got, M):
        tol = M * self.e32[fam]
        ref = self.t[(fam, layer)]
        if fam in SLICE_AXES:
            got64 = np.asarray(got, np.float64)
            err = np.abs(got64 - ref).max(axis=SLICE_AXES[fam])
            den = np.abs(ref).max(axis=SLICE_AXES[fam])
            return (err > tol * den + R.UNDERFLOW) | ~np.isfinite(err)
        return R.componentwise_failures(got, ref, R.scale_of(self.full, fam, layer), tol)

    def zero_positions(self, fam, layer):
        """boolean array: where the factors make the reference an exact zero (a dropped unit; dh / dx at a dropped position)"""
        L = self.config['n_layers']
        n = self.cache['B'] * self.config['max_len']
        if fam == 'drop':
            return self.f[layer] == 0
        if fam == 'dx':
            return self.f[0].reshape(n, -1) == 0
        if fam == 'dh':
            return self.f[1].reshape(n, -1) == 0
        raise KeyError(fam)
