"""Restatement of oracle.lstm_oracle.backward that keeps what the oracle throws away (TEST INFRASTRUCTURE ONLY).

backward_full() does the oracle's arithmetic in the oracle's order -- in fp64 its gradients are the oracle's bit for bit
(tests/test_componentwise_cpu.py) -- for any number of layers, and also returns

  * the intermediates of the pass: dlogits, dz of every layer, dx (the embedding slices), dh (the gradient that arrives at
    layer 0's chain from above), all in the oracle's row order b*T + t;
  * for every tensor that is a sum of products, G = sum_r a_r b_r, the scale S = sum_r |a_r| |b_r| against which a
    componentwise error bound |got - ref| <= tol * S is stated (Higham, Accuracy and Stability of Numerical Algorithms,
    section 3.5: a floating-point inner product errs by a small multiple of u * S, whatever the order of the additions).

The measures themselves (componentwise_ratio, slice_ratio), the fp32-restatement yardstick e32 and the bound
M * e32 (class Reference) live here too, so that the CPU and the GPU tests use one definition.

The padding-masked pass is the same arithmetic with per-row weights: backward_full and Reference take the 0 / 1
weights of the rows, in the oracle's row order b*T + t.  A masked row then has S == 0 in dlogits, dh, dx, and an all-zero reference
in every gate block of its rows of dz -- so the measures hold everything the device writes there to exact zeros.
"""
import numpy as np

from oracle import lstm_oracle as O

UNDERFLOW = 1e-30          # absolute slack for fp32 underflow, added to every bound; nothing else is


# ----------------------------------------------------------------------------- the backward pass, with its intermediates
def backward_full(params, cache, config, weights=None):
    """-> dict(grads, aux, dlogits [n,V1], dz [L x [n,4H]], dx [n,E], dh [n,H], scales {name: S}).

    weights: None (the oracle's loss, every row counts), or the rows' 0 / 1 weights of the padding-masked loss, [n] in the oracle's
    row order b*T + t (masked_ref.mask_of).  Row r then enters with mask_r / (n_valid + 1e-12), n_valid = sum(mask), in the division
    form of masked_ref.masked_backward, whose gradients these are bit for bit:
        dlogits = (p - onehot) * mask / (n_valid + 1e-12),   scales['dlogits'] = (p + onehot) * mask / (n_valid + 1e-12),
    and every other scale follows from |dlogits| as without weights.  A masked row has S == 0 in dlogits, dh and dx, and zeros in
    its rows of every dz.  Without weights every returned array is bit-identical to what this function returned before it took them."""
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
        scales['dlogits'] = s_dlogits / dtype.type(n + 1e-12)             # (p + onehot) / n
        dlogits = p / dtype.type(n + 1e-12)
    else:
        mask = np.asarray(weights).reshape(n).astype(dtype)
        assert np.all((mask == 0) | (mask == 1)) and mask.any(), 'the weights of the padding-masked loss are 0 / 1, not all 0'
        n_valid = int(mask.sum())
        scales['dlogits'] = s_dlogits * mask[:, None] / dtype.type(n_valid + 1e-12)
        dlogits = p * mask[:, None] / dtype.type(n_valid + 1e-12)
    a_dl = np.abs(dlogits)
    grads['softmax_w'] = cache['out'].T.dot(dlogits)
    grads['softmax_b'] = dlogits.sum(axis=0)
    scales['softmax_w'] = np.abs(cache['out']).T.dot(a_dl)
    scales['softmax_b'] = a_dl.sum(axis=0)
    dtop = dlogits.dot(params['softmax_w'].T).reshape(B, T, H)
    s_dtop = a_dl.dot(np.abs(params['softmax_w']).T)                      # scale of what arrives at the top layer's chain

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
        if l == 0:                                                        # the input of layer 0's chain
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
        dtop = dzf.dot(K[:n_in].T).reshape(B, T, n_in)
        s_dtop = a_dz.dot(np.abs(K[:n_in]).T)

    dx = dtop.reshape(n, -1)
    demb = np.zeros_like(params['embedding'])
    np.add.at(demb, cache['X'].reshape(n), dx)
    grads['embedding'] = demb
    # NOT the scatter-add of |dx|: dx itself cancels (a sum over 4H gate columns), the product form does not hide that
    s_emb = np.zeros_like(params['embedding'])
    np.add.at(s_emb, cache['X'].reshape(n), s_dtop)
    scales['embedding'] = s_emb
    scales['dx'] = s_dtop
    scales['dh'] = s_dh
    aux = dict(embedding_slices_sq=float((dx.astype(np.float64) ** 2).sum()))
    return dict(grads=grads, aux=aux, dlogits=dlogits, dz=dz_layers, dx=dx, dh=dh, scales=scales)


# ----------------------------------------------------------------------------- the measures
def componentwise_ratio(got, ref, S):
    """-> the array |got - ref| / S, 0 where S == 0 (those elements are held to exact zero by componentwise_failures)"""
    got, ref, S = (np.asarray(a, np.float64) for a in (got, ref, S))
    err = np.abs(got - ref)
    out = np.zeros_like(err)
    np.divide(err, S, out=out, where=S > 0)
    return out


def componentwise_failures(got, ref, S, tol):
    """Boolean array of the elements that miss |got - ref| <= tol * S + 1e-30, or are not exactly 0.0 where S == 0.
    EVERY element is in one of the two checks."""
    got, ref, S = (np.asarray(a, np.float64) for a in (got, ref, S))
    assert got.shape == ref.shape == S.shape, (got.shape, ref.shape, S.shape)
    bad = np.abs(got - ref) > tol * S + UNDERFLOW
    return np.where(S > 0, bad, got != 0.0) | ~np.isfinite(got)


def slice_ratio(got, ref, axes):
    """Norm-wise error per slice, max|err| / max|ref| over `axes`; a slice whose reference is all zero (h_0, c_0; with weights
    every gate block of a masked (t, b) row of dz) counts max|err| / 1e-30, so anything but exact zeros there is far outside every
    bound."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref).max(axis=axes)
    den = np.abs(ref).max(axis=axes)
    return err / np.maximum(den, UNDERFLOW)


# ----------------------------------------------------------------------------- the two reference passes of one episode
COMPONENTWISE = ('logits', 'lse', 'ce', 'dlogits', 'dh', 'dx', 'softmax_w', 'softmax_b', 'kernel', 'bias', 'embedding')
SLICEWISE = ('hs', 'cs', 'dz')
FAMILIES = COMPONENTWISE + SLICEWISE


def _tensors(params, X, Y, config, weights=None):
    """every checked tensor of one forward + backward pass, by (family, layer or None), oracle row order; with weights the loss
    is the padding-masked one, sum of the scored rows' ce / (n_valid + 1e-12) (masked_ref.masked_loss)"""
    loss, cache = O.forward(params, X, Y, config)
    full = backward_full(params, cache, config, weights)
    if weights is not None:
        mask = np.asarray(weights).reshape(-1)
        loss = (cache['ce'] * mask.astype(cache['ce'].dtype)).sum() / (int(mask.sum()) + 1e-12)
    H, T, B = config['hidden_size'], config['max_len'], cache['B']
    t = {('logits', None): cache['logits'], ('lse', None): cache['lse'], ('ce', None): cache['ce'],
         ('dlogits', None): full['dlogits'], ('dh', None): full['dh'], ('dx', None): full['dx'],
         ('softmax_w', None): full['grads']['softmax_w'], ('softmax_b', None): full['grads']['softmax_b'],
         ('embedding', None): full['grads']['embedding']}
    for l in range(config['n_layers']):
        t[('kernel', l)] = full['grads']['kernel_%d' % l]
        t[('bias', l)] = full['grads']['bias_%d' % l]
        t[('hs', l)] = cache['layers'][l]['hs']                                        # [T+1, B, H]
        t[('cs', l)] = cache['layers'][l]['cs']
        t[('dz', l)] = full['dz'][l].reshape(B, T, 4, H)                               # [B, T, gate, H]
    return float(loss), cache, full, t


def scale_of(full, fam, layer):
    return full['scales'][fam if layer is None else '%s_%d' % (fam, layer)]


SLICE_AXES = {'hs': (2,), 'cs': (2,), 'dz': (3,)}      # one (t, b) row of H units; for dz one gate block of it


def measure(fam, layer, got, ref_t, ref_full):
    """the family's measure of `got` against the fp64 reference, as an array (one number per element / per slice)"""
    ref = ref_t[(fam, layer)]
    if fam in SLICEWISE:
        return slice_ratio(got, ref, SLICE_AXES[fam])
    return componentwise_ratio(got, ref, scale_of(ref_full, fam, layer))


class Reference(object):
    """fp64 oracle pass + its fp32 restatement (same parameters, same episode) of one shape; e32[family] = the fp32 pass's
    error in the family's own measure, maximised over the family (all layers): what plain fp32 arithmetic gives.  The
    device is held to M * e32 -- a yardstick that comes from the reference alone, never from the code under test.
    weights: as backward_full's; both passes take the same ones."""

    def __init__(self, params64, X, Y, config, weights=None):
        self.config, self.X, self.Y, self.weights = config, X, Y, weights
        self.params = params64
        self.loss, self.cache, self.full, self.t = _tensors(params64, X, Y, config, weights)
        p32 = {k: v.astype(np.float32) for k, v in params64.items()}
        _, _, _, t32 = _tensors(p32, X, Y, config, weights)
        self.e32 = {}
        for (fam, layer), a32 in t32.items():
            assert a32.dtype == np.float32, (fam, a32.dtype)
            if fam in COMPONENTWISE:       # where S == 0 the fp32 pass holds an exact zero too (no term contributes)
                assert np.all(a32[scale_of(self.full, fam, layer) == 0] == 0), fam
            self.e32[fam] = max(self.e32.get(fam, 0.0), float(measure(fam, layer, a32, self.t, self.full).max()))

    def ratio(self, fam, layer, got):
        """worst measure of `got` in units of e32 (what the tables of tests/COMPONENTWISE.md list), and where it sits"""
        m = measure(fam, layer, got, self.t, self.full)
        i = np.unravel_index(int(np.argmax(m)), m.shape)
        return float(m[i]) / self.e32[fam], i

    def failures(self, fam, layer, got, M):
        """boolean array: elements (slices) of `got` outside M * e32 -- or not exactly zero where nothing contributes"""
        tol = M * self.e32[fam]
        ref = self.t[(fam, layer)]
        if fam in SLICEWISE:
            got64 = np.asarray(got, np.float64)
            err = np.abs(got64 - ref).max(axis=SLICE_AXES[fam])
            den = np.abs(ref).max(axis=SLICE_AXES[fam])
            return (err > tol * den + UNDERFLOW) | ~np.isfinite(err)
        return componentwise_failures(got, ref, scale_of(self.full, fam, layer), tol)


# ----------------------------------------------------------------------------- the shapes both test files run
# (config overrides, N, K, Q, episode seed): taken from SHAPES of tests/test_gpu_parity.py -- the smallest shapes that still
# reach each kernel family -- plus the long Zipf episode of its two-level embedding-gradient test
CW_SHAPES = [
    (dict(), 2, 2, 1, 3),                                                                           # B = 6: one partial M tile
    (dict(hidden_size=20, embedding_size=10, input_size=50, max_len=7), 1, 1, 1, 3),               # nothing a multiple of 16 or 4
    (dict(hidden_size=48, embedding_size=24, input_size=301, max_len=9), 5, 5, 4, 3),              # B = 45
    (dict(hidden_size=32, embedding_size=12, input_size=77, max_len=6, n_layers=2), 3, 2, 2, 3),   # stacked
    (dict(hidden_size=128, embedding_size=16, input_size=80, max_len=5), 20, 1, 4, 3),             # 7 row tiles on the persistent chain
    (dict(hidden_size=200, embedding_size=24, input_size=90, max_len=7), 5, 5, 4, 3),              # padded to 256: pads beside live units
    (dict(hidden_size=256, embedding_size=16, input_size=70, max_len=6), 5, 5, 4, 3),              # slice kernels
    (dict(hidden_size=512, embedding_size=16, input_size=60, max_len=6), 5, 5, 4, 3),              # XCD-local kernels, fp32
    (dict(hidden_size=512, embedding_size=16, input_size=60, max_len=5), 20, 1, 4, 3),             # ... bf16-split (100 rows > 64)
    (dict(hidden_size=1024, embedding_size=16, input_size=60, max_len=4, n_layers=2), 2, 1, 1, 3),  # pair kernels, stacked
    (dict(hidden_size=16, embedding_size=8, input_size=7000, max_len=4), 2, 1, 1, 3),              # 12-register cross-entropy kernel
    (dict(hidden_size=16, embedding_size=8, input_size=12500, max_len=4), 2, 1, 1, 3),             # 3-pass cross-entropy kernel
    (dict(hidden_size=320, embedding_size=250, input_size=300, max_len=6), 5, 5, 4, 3),            # E = 250 pads to one 256-row tile
    (dict(hidden_size=64, embedding_size=40, input_size=500, max_len=96, n_layers=1), 5, 3, 3, 17),  # two-level embedding gradient
]


def shape_id(shape):
    over, N, K, Q, seed = shape
    return '-'.join(['%s%s' % (k[0].upper(), v) for k, v in sorted(over.items())] + ['%dx%dx%d' % (N, K, Q)]) or 'default'


def episode(cfg, N, K, Q, seed):
    (sup, qry), = O.synthetic_episodes(1, N, K, Q, cfg['max_len'], cfg['input_size'], seed=seed, realistic=True)
    return sup, qry
