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


# ----------------------------------------------------------------------------- forced kernel families and row edges
# What tests/test_gpu_forced_componentwise.py runs and tests/test_forced_componentwise_cpu.py builds the references of: the
# recurrence kernels a default run only picks at some row counts, and the ones behind the knobs fsmg_create reads.  A case is
# (environment, config overrides, N, K, Q, episode seed); the row count is N * (K + Q).  CW_SHAPES stays what it is.
_NKQ = {1: (1, 0, 1), 4: (2, 1, 1), 6: (2, 2, 1), 9: (3, 2, 1), 12: (3, 2, 2), 16: (4, 2, 2), 32: (8, 2, 2), 33: (11, 2, 1), 45: (5, 5, 4),
        48: (8, 3, 3), 49: (7, 4, 3), 64: (16, 2, 2), 65: (13, 3, 2), 70: (10, 4, 3), 80: (10, 4, 4), 96: (16, 3, 3), 100: (20, 1, 4),
        128: (16, 4, 4), 129: (43, 2, 1)}


def _case(hidden, B, max_len=None, env=None, **over):
    """hidden x B rows with the small dims every case shares; a row count without an entry above (17, 97) is N songs of an empty support
    set and one query song each.  max_len 3 -- two recurrent steps: h_{t-1} and the dc carry are live -- from 9 rows on.  Below, three
    steps leave a weight-gradient element with one to a dozen terms, a unit that is small in all of them carries its whole S, and e32
    of kernel rises to 3e-5 .. 1.6e-4 (the "all lengths 1" effect of tests/COMPONENTWISE.md): 4 and 6 rows take 6 steps, 1 row 12,
    which brings it back to 1e-6 .. 7e-6 (tests/test_forced_componentwise_cpu.py holds every shape below 2e-5)."""
    N, K, Q = _NKQ.get(B, (B, 0, 1))
    assert N * (K + Q) == B
    if max_len is None:
        max_len = 12 if B == 1 else 6 if B < 9 else 3
    cfg = dict(hidden_size=hidden, embedding_size=16, input_size=60, max_len=max_len, n_layers=1)
    cfg.update(over)
    return (dict(env or {}), cfg, N, K, Q, 3)


# (a) the row edges of the default dispatch, no knob set: every row count at which a kernel's row geometry changes
FORCED_ROW_EDGES = \
    [_case(512, B) for B in (1, 9, 32, 33, 64, 65, 96, 97, 128, 129)] + \
    [_case(1024, B) for B in (1, 16, 17, 32, 33, 48, 49, 64, 65)] + \
    [_case(256, B) for B in (1, 16, 17, 64, 65, 128, 129)] + \
    [_case(128, B) for B in (16, 17, 48, 49)] + \
    [(dict(), dict(hidden_size=32, embedding_size=16, input_size=130, max_len=5), 10, 4, 3, 3)]      # B = 70 of parity SHAPES: k_lstm_fwd_patch
# (b) one launch per time step
_PS = dict(FSMG_PERSISTENT='0')
FORCED_PER_STEP = [_case(64, 12, env=_PS), _case(128, 45, env=_PS), _case(128, 100, env=_PS), _case(200, 45, env=_PS),
                   _case(512, 45, env=_PS), _case(512, 100, env=_PS), _case(1024, 4, env=_PS, n_layers=2), _case(1024, 49, env=_PS)]
# (c) the column-split persistent kernels where the XCD-local ones are the default, and the all-row-tiles forward kernel
FORCED_COLUMN_SPLIT = \
    [_case(h, B, env=dict(FSMG_XCD='0')) for h in (256, 512) for B in (45, 100)] + \
    [_case(1024, B, env=dict(FSMG_XCD_PAIR=m), n_layers=L) for m in ('0', '1') for B, L in ((4, 2), (45, 1))] + \
    [_case(128, 45, env=dict(FSMG_FWD_RT='1')), _case(64, 64, env=dict(FSMG_FWD_RT='1'))]
# (d) the other arithmetic of the XCD-local kernels
FORCED_XCD_ARITH = \
    [_case(512, 6, env=dict(FSMG_XCD_BX3='1')), _case(512, 45, env=dict(FSMG_XCD_BX3='1')), _case(512, 100, env=dict(FSMG_XCD_BX3='0'))] + \
    [_case(1024, 4, env=dict(FSMG_XCD_BX3='1', **v), n_layers=2) for v in (dict(), dict(FSMG_XCD_VARIANT='32'), dict(FSMG_XCD_VARIANT='176'))]
# (e) the XCD-partitioned order and, on the same shapes against the same reference, the serial one.  Which halves a shape can take is
# decided by expected_dispatch below: 45 x 6 rows the forward pair alone (dW's K split needs 512 rows), 100 rows NEITHER (the packed
# chain would sit on 7 XCDs, the order wants at least three for the GEMMs), 80 x 7 rows both, and 45 x 46 rows at E = 250 -- the
# smallest shape of tests/test_xov_dk_tail.py -- both with the merged dK in dW's clean-up launch.
_XOV_SHAPES = [_case(512, 45, max_len=6), _case(512, 100, max_len=6), _case(512, 80, max_len=7),
               _case(512, 45, max_len=46, embedding_size=250, input_size=1800)]
FORCED_XOV = [(dict(FSMG_XCD_OVERLAP=o, FSMG_XOV_PARTS='7'),) + c[1:] for c in _XOV_SHAPES for o in ('1', '0')]
# (f) recovery from the designed software time-out
FORCED_RECOVERY = _case(512, 45, max_len=4)
FORCED_CASES = FORCED_ROW_EDGES + FORCED_PER_STEP + FORCED_COLUMN_SPLIT + FORCED_XCD_ARITH + FORCED_XOV


def forced_shape(case):
    """the CW_SHAPES form of a case (its reference does not depend on the environment)"""
    return case[1:]


def forced_id(case):
    env = '+'.join('%s=%s' % (k[5:], v) for k, v in sorted(case[0].items()))
    return (env + '|' if env else '') + shape_id(forced_shape(case))


# The dispatch of csrc/api_forward.hip forward(), api_backward.hip backward(), fsmg_model.h use_xcd and api_schedule.hip
# choose_schedule, restated for one train pass of a FRESH handle created for max_sequences = B rows with the default GEMM arithmetic:
# which recurrence kernel each direction takes and how many launches fsmg_stats then counts.  Every function below is the C++ one of
# the same name (lstm_step.hip, lstm_xcd.hip); the tests assert the device's counters against it.
def _cdiv(a, b):
    return -(-a // b)


def lstm_fwd_chain_supported(B, Hp):
    ng = Hp >> 4
    if Hp & 15 or ng & 3 or (ng >> 2) not in (1, 2, 4, 8, 16):
        return False
    return (4 * Hp // 16) * _cdiv(B, 16) <= 256 * (2 if (ng >> 2) >= 16 else 4) * 9 // 10


def lstm_fwd_chain_rt_supported(B, Hp):
    ng = Hp >> 4
    if Hp & 15 or ng & 3 or (ng >> 2) not in (1, 2, 4, 8, 16):
        return False
    return 2 <= _cdiv(B, 16) <= 4 and 4 * Hp // 16 <= 256 * (1 if (ng >> 2) >= 16 else 3)


def lstm_bwd_chain_supported(B, Hp):
    ng = (4 * Hp) >> 4
    if Hp & 15 or ng & 7 or (ng >> 3) not in (2, 4, 8, 16):
        return False
    return (Hp // 16) * _cdiv(B, 16) <= 256 * 3 // 4


def lstm_bwd_rs_supported(B, Hp):
    return Hp % 128 == 0 and Hp // 128 in (1, 2, 4, 8) and (Hp // 16) * _cdiv(B, 16) <= 256 * 9 // 10


def xcd_row_groups(B, Hp):
    if Hp == 1024:
        return _cdiv(_cdiv(B, 4), 4)                  # one weight copy per XCD pair
    if Hp == 256:
        return _cdiv(_cdiv(B, 16), 4)                 # sixteen slices
    rg = _cdiv(_cdiv(B, 8), 4)
    return 4 if rg == 3 else rg


def lstm_xcd_supported(B, Hp):
    return Hp in (256, 512, 1024) and B >= 1 and xcd_row_groups(B, Hp) <= (2 if Hp == 256 else 4)


def lstm_xcd_bx3_pays(B, Hp):
    return Hp in (512, 1024) and xcd_row_groups(B, Hp) >= 3


def lstm_xcd16_packed_rows(B, Hp):
    nx = _cdiv(B, 16)
    return _cdiv(B, nx) if 1 <= nx <= (4 if Hp == 1024 else 8) else 0


def xov_first_free(B, Hp):
    rpx = lstm_xcd16_packed_rows(B, Hp)
    return (2 if Hp == 1024 else 1) * _cdiv(B, rpx) if rpx > 0 else 8


def padded_hidden(H):
    """api_layout.hip compute_dims: a multiple of 16, or of 64 where only that admits the persistent kernels at a third more columns at most"""
    h16, h64 = _cdiv(H, 16) * 16, _cdiv(H, 64) * 64
    if not lstm_fwd_chain_supported(45, h16) and lstm_fwd_chain_supported(45, h64) and 3 * h64 <= 4 * h16 and h16 not in (256, 512, 1024):
        return h64
    return h16


XCD_MAX_ROWS = 128        # fsmg_model::xcd_max_rows
XOV_CTL = 8192            # fsmg_model::XOV_CTL: queue words of a work-queue GEMM


def expected_dispatch(cfg, B, env, persist_now=None):
    """-> dict(Hp, fwd, bwd, xcd_launches, persistent_launches, step_launches, xcd_bx3, xov (the pass takes the XCD-partitioned order:
    xcd_partitioned[2]), xov_fwd, xov_bwd, dw_split, dk_tail) of ONE forward_backward on a fresh handle created for B rows.
    persist_now=False: the handle is inside a fallback period (fsmg_model::persist is off, what fsmg_create decided stays)."""
    H, T, L, E, V1 = cfg['hidden_size'], cfg['max_len'], cfg['n_layers'], cfg['embedding_size'], cfg['input_size'] + 1
    Hp, Ep, V1p = padded_hidden(H), _cdiv(E, 16) * 16, _cdiv(V1, 4) * 4
    assert env.get('FSMG_GEMM', 'bx3') == 'bx3' and 'FSMG_OVERLAP' not in env
    assert V1 < 8 * H * L, 'the two-stream order (chunked chains) is not restated here'
    persist_cfg = env.get('FSMG_PERSISTENT', '1') != '0'
    xcd_knob = env.get('FSMG_XCD', '1') != '0'
    pair_mode = max(0, min(2, int(env.get('FSMG_XCD_PAIR', 2))))
    force_rt = env.get('FSMG_FWD_RT', '0') != '0'
    images = persist_cfg and xcd_knob and lstm_xcd_supported(1, Hp)         # fsmg_create: the XCD-local weight images exist
    # fsmg_create: the order by name, else AUTO's rule (cfg-B-like shapes only: T >= 32 and 320 projection tiles)
    rpx0 = lstm_xcd16_packed_rows(B, 512)
    items0 = _cdiv(T * B, 256) * _cdiv(V1p, 256)
    xov = images and Hp == 512 and L == 1 and rpx0 > 0 and _cdiv(B, rpx0) <= 5 and B >= 16 and T >= 32 and items0 >= 320 and 4 + items0 <= XOV_CTL
    if 'FSMG_XCD_OVERLAP' in env:
        xov = int(env['FSMG_XCD_OVERLAP']) != 0
    parts = max(1, min(7, int(env['FSMG_XOV_PARTS']))) if 'FSMG_XOV_PARTS' in env else (2 if Hp == 1024 and images else 3)
    # the format of the XCD-local kernels: fsmg_create, then select_xcd_format per train pass at hidden 1024
    bx3 = False
    if images:
        bx3 = (lstm_xcd_bx3_pays(B, Hp) and B <= XCD_MAX_ROWS) or (xov and Hp == 512)
        if 'FSMG_XCD_BX3' in env:
            bx3 = int(env['FSMG_XCD_BX3']) != 0 and Hp in (512, 1024)
        elif Hp == 1024:
            bx3 = lstm_xcd_bx3_pays(B, Hp) and B <= XCD_MAX_ROWS
    persist = persist_cfg if persist_now is None else persist_now

    def use_xcd(backward):
        if Hp == 1024 and pair_mode < (2 if backward else 1):
            return False
        return persist and images and B <= XCD_MAX_ROWS and lstm_xcd_supported(B, Hp)

    # choose_schedule: the packed chains must leave three XCDs (hidden 1024: a pair) to the GEMMs
    rpx = lstm_xcd16_packed_rows(B, Hp)
    xov_call = bool(xov and ((Hp == 512 and L == 1) or Hp == 1024) and bx3 and use_xcd(False) and rpx > 0 and
                    xov_first_free(B, Hp) <= (6 if Hp == 1024 else 5))
    xov_fwd = xov_call and bool(parts & 1) and 4 + _cdiv(T * B, 256) * _cdiv(V1p, 256) <= XOV_CTL
    dw_split = max(1, min(4, 16, T * B // 256)) if xov_call and parts & 2 and use_xcd(True) else 1     # fsmg_model::xov_dw_split = 4
    xov_bwd = dw_split > 1 and 4 + _cdiv(Hp, 256) * _cdiv(V1p, 256) * dw_split <= XOV_CTL
    # the merged dK as the tail of dW's clean-up launch: one 512-unit layer, Ep a multiple of 256, and the 256-tile kernel's own rule
    # for a merged dK (use_h_gemm: fewer than 64 tiles -> K >= 2048 rows)
    tiles = _cdiv(Ep + Hp, 256) * _cdiv(4 * Hp, 256)
    dk_tail = bool(xov_bwd and L == 1 and Hp == 512 and Ep % 256 == 0 and (T * B >= 896 if tiles >= 64 else (T * B >= 2048 and tiles >= 16)))

    if use_xcd(False):
        fwd = 'xcd'
    elif persist and not force_rt and lstm_fwd_chain_supported(B, Hp):
        fwd = 'chain'
    elif persist and lstm_fwd_chain_rt_supported(B, Hp):
        fwd = 'chain_rt'
    else:
        fwd = 'patch' if _cdiv(B, 16) >= 4 and (4 * Hp // 16) % 2 == 0 else 'step'          # launch_lstm_fwd_step
    # ensure_scratch: the reduce-scatter inboxes exist where k_lstm_bwd_rs takes 16 rows at this Hp, the all-gather buffer only otherwise
    inbox = persist and lstm_bwd_rs_supported(16, Hp)
    if use_xcd(True):
        bwd = 'xcd'
    elif inbox and lstm_bwd_rs_supported(B, Hp):
        bwd = 'rs'
    elif persist and not inbox and lstm_bwd_chain_supported(B, Hp):
        bwd = 'chain'
    else:
        bwd = 'step'
    # one launch per layer and direction (no time chunks without the two-stream order), T of them on per-step launches
    n = dict(xcd=0, persistent=0, step=0)
    for k in (fwd, bwd):
        n['xcd' if k == 'xcd' else 'step' if k in ('step', 'patch') else 'persistent'] += L * (T if k in ('step', 'patch') else 1)
    return dict(Hp=Hp, fwd=fwd, bwd=bwd, xcd_launches=n['xcd'], persistent_launches=n['persistent'], step_launches=n['step'],
                xcd_bx3=bool(bx3), xov=xov_call, xov_fwd=bool(xov_fwd), xov_bwd=bool(xov_bwd), dw_split=dw_split, dk_tail=dk_tail)
