"""The decode path's kernels against fp64, element by element: the reference, the measure and an fp32 stand-in of the kernels.

Every decode entry point advances through advance() (csrc/api_decode.hip): k_gen_cell per layer, k_gen_logits, then a row kernel that
reads the row through row_max_lse (csrc/decode.hip).  tests/test_gpu_decode_componentwise.py observes them through the public calls
only (FsmgModel.new_state / feed, DecodeState.get / set / gather); tests/test_decode_componentwise_cpu.py runs the same checks on
the stand-in below and on planted mistakes.

ONE CELL STEP.  The state (h uniform in (-1, 1), c uniform in (-2, 2), fp32) and one pending token per row are set, one token is fed,
the state is read back.  Layer l of the reference is one fp64 step from the inputs the device itself had: x = the embedding row of the
pending token (l = 0) or the device's own new h of layer l - 1 (l > 0), h and c the values that were set.  With
z_g = sum_k x_k Kx[k, g] + sum_k h_k Kh[k, g] + b_g (+ 1 for the forget gate),  i = sigmoid(z_i), j = tanh(z_j), f = sigmoid(z_f + 1),
o = sigmoid(z_o),  c' = c f + i j,  h' = tanh(c') o,  the first-order propagated scales are

    A_g  = sum_k |x_k Kx[k, g]| + sum_k |h_k Kh[k, g]| + |b_g|   (+ 1 for the forget gate: the constant is one more term)
    d_i  = i (1 - i) A_i + i        d_j = (1 - j^2) A_j + |j|        d_f = f (1 - f) A_f + f        d_o = o (1 - o) A_o + o
    S_c  = |c| d_f + |j| d_i + i d_j + |c f| + |i j|
    S_h  = o (1 - tanh(c')^2) S_c + |tanh(c')| d_o + |h'|

d_g is the magnitude of the products of the gate's pre-activation carried through the activation's derivative, plus the gate's own
value (the activation's own rounding); S_c carries them through c' = c f + i j and adds the magnitudes of its two terms; S_h carries S_c
and d_o through h' = tanh(c') o and adds |h'|.  The measure of families `c` and `h` is |got - ref| / S per element; pad units
(u >= hidden_size) have S = 0 and are compared with 0.0.

A ROW OF LOGITS.  The state is gathered to n rows that are copies of one row and row v is fed token cols[v] with log-probs, so row v
returns z[cols[v]] - lse of the same h; the reference is h_dev . softmax_w + softmax_b - logsumexp in fp64 over all V1 columns from the
device's own new top-layer h.  Family `lp`: |got - ref| / S_v with

    Z_v = sum_k |h_k W[k, v]| + |b_v|        S_v = Z_v + sum_u p_u Z_u + |lse|        p = softmax(z)

and sum_v exp(lp_v) = 1 within M e32 sum_v p_v S_v: the first-order effect of every column being off by its own bound.

THE BOUND is M * e32, M = 8 (tests/COMPONENTWISE.md), e32 the same measure of a plain fp32 numpy restatement of the same step from the
same inputs, maximised over the family (all layers, all elements), never below 2^-24: one rounding.
"""
import numpy as np

from oracle import lstm_oracle as O

M = 8
U = 2.0 ** -24
GEN_CH = 16                  # csrc/decode.hip: k per lane held in registers at a time
GEN_ROWS = 64                # rows per workgroup, four row tiles of 16
PICK_LDS_FLOATS = 32 * 1024  # rows up to this many columns are staged in LDS
SWEEP = 8 * 1024             # columns one iteration of row_max_lse's first sweep covers
MAX_CHECKED = 256
FAMILIES = ('c', 'h')


def round_up(a, b):
    return (a + b - 1) // b * b


def config(E, H, L, V):
    return dict(name='lstm_baseline', seed=1234, input_size=V, max_len=4, embedding_size=E, hidden_size=H, n_layers=L, lr=5e-3,
                max_grad_norm=5, n_decay=10000)


# ---------------------------------------------------------------------------------------------------------------- the cases
# (id, E, H, L, the padded hidden sizes the default rule may give, what the case reaches).  Ep = round_up(E, 16); vocabulary 199 + the
# start word, so that up to 129 rows read distinct tokens.
CELL_V = 199
CELL_CASES = [
    ('E8-H16-L1', 8, 16, 1, (16,)),            # m = 1 in both segments
    ('E20-H21-L2', 20, 21, 2, (32,)),          # H % 4 != 0, pad units; layer 1 reads the layer below's h with in_dim = Hp
    ('E250-H200-L1', 250, 200, 1, (208, 256)),  # Ep 256: m = 16, exactly one register chunk
    ('E260-H260-L1', 260, 260, 1, (272, 320)),  # Ep 272: m = 17; Hp 272 or 320: m = 17 or 20 -- a full chunk plus a partial one
    ('E16-H512-L1', 16, 512, 1, (512,)),       # m = 32
    ('E16-H1024-L2', 16, 1024, 2, (1024,)),    # m = 64
]
CELL_ROWS = 17
ROWS_CASE = CELL_CASES[1]
ROW_COUNTS = [1, 15, 16, 17, 33, 63, 64, 65, 129]  # nrt 1 .. 4 (33 rows: three row tiles), gridDim.y 1 .. 3 with a partial last block

# full logit rows through the gather: (E, H, V1); the row count of each is V1
LP_FULL = [(8, 16, v) for v in (2, 15, 16, 17, 98, 257, 1025)] + [(16, 512, 1025)]
# checked columns only, at H16: V1 -> whether row_max_lse stages the row in LDS (V1 <= PICK_LDS_FLOATS, launch_row_kernel)
LP_WIDE = [(8193, True), (32768, True), (32769, False), (50001, False)]


def cell_id(case):
    return case[0]


def staged(V1):
    return V1 <= PICK_LDS_FLOATS


# ---------------------------------------------------------------------------------------------------------------- seeded inputs
def seeded_params(cfg, seed=0):
    """fp32 parameters whose gate pre-activations have a spread near 1 on seeded_state's inputs: the x part and the h part of a
    pre-activation each have variance 0.4 (x: embedding rows uniform in (-1, 1), variance 1/3; above layer 0 the h below, variance
    about 0.1), the bias is uniform in (-0.5, 0.5); the logits' spread is about 1.5"""
    rng = np.random.RandomState(seed)
    d = O.model_dims(cfg)
    H = d['H']
    p = {}
    for name, shape in O.param_shapes(cfg):
        if name == 'embedding':
            v = rng.uniform(-1.0, 1.0, shape)
        elif name.startswith('kernel_'):
            in_r = shape[0] - H
            var_x = 1.0 / 3.0 if name == 'kernel_0' else 0.1
            a, b = np.sqrt(1.2 / (in_r * var_x)), np.sqrt(3.6 / H)
            v = np.concatenate([rng.uniform(-a, a, (in_r, shape[1])), rng.uniform(-b, b, (H, shape[1]))])
        elif name.startswith('bias_'):
            v = rng.uniform(-0.5, 0.5, shape)
        elif name == 'softmax_w':
            s = np.sqrt(67.0 / H)
            v = rng.uniform(-s, s, shape)
        else:
            v = rng.uniform(-1.0, 1.0, shape)
        p[name] = v.astype(np.float32)
    return p


def seeded_state(cfg, R, seed=0, copies=False):
    """-> pending tokens int32 [R] (0, input_size - 1 and the start word among them; distinct while R <= V1), h, c fp32 [L, R, H]"""
    rng = np.random.RandomState(1000 + seed)
    d = O.model_dims(cfg)
    L, H, V1 = d['L'], d['H'], d['V1']
    h = rng.uniform(-1.0, 1.0, (L, R, H)).astype(np.float32)
    c = rng.uniform(-2.0, 2.0, (L, R, H)).astype(np.float32)
    special = [0, V1 - 2, V1 - 1]
    rest = [t for t in rng.permutation(V1) if t not in special]
    tok = np.array((special + rest * (R // max(len(rest), 1) + 1))[:R], np.int32)
    if R >= 3:
        tok[[1, R - 1]] = tok[[R - 1, 1]]      # an edge token in the last row as well
    if copies:
        r0 = min(2, R - 1)
        h, c, tok = np.repeat(h[:, r0:r0 + 1], R, 1), np.repeat(c[:, r0:r0 + 1], R, 1), np.repeat(tok[r0:r0 + 1], R)
    return tok, np.ascontiguousarray(h), np.ascontiguousarray(c)


def checked_columns(V1, seed=0):
    """the columns of a wide row that are fed, at most MAX_CHECKED: 0 .. 16, the 17 around every multiple of the sweep's 8192, 32 760 ..
    min(V1, 32 776) - 1, the last 17, seeded random ones for the rest; every column when there are no more than that"""
    if V1 <= MAX_CHECKED:
        return np.arange(V1, dtype=np.int32)
    cols = set(range(17))
    for edge in range(SWEEP, V1 + 9, SWEEP):
        cols.update(range(edge - 8, edge + 9))
    cols.update(range(PICK_LDS_FLOATS - 8, min(V1, PICK_LDS_FLOATS + 8)))
    cols.update(range(V1 - 17, V1))
    cols = set(v for v in cols if 0 <= v < V1)
    assert len(cols) <= MAX_CHECKED
    rng = np.random.RandomState(2000 + seed)
    for v in rng.permutation(V1):
        if len(cols) >= MAX_CHECKED:
            break
        cols.add(int(v))
    return np.array(sorted(cols), np.int32)


# ---------------------------------------------------------------------------------------------------------------- the reference
def _sigmoid(x):
    one = x.dtype.type(1)
    return one / (one + np.exp(-x))


def layer_step(params, l, H, x, h, c, dtype=np.float64, scales=False):
    """one layer, one position: x [R, in], h, c [R, H] -> h', c' (and S_h, S_c, the pre-activations z) in `dtype` arithmetic"""
    K, b = params['kernel_%d' % l].astype(dtype), params['bias_%d' % l].astype(dtype)
    xh = np.concatenate([x, h], axis=1).astype(dtype)
    c = c.astype(dtype)
    z = xh.dot(K) + b
    i, j = _sigmoid(z[:, :H]), np.tanh(z[:, H:2 * H])
    f, o = _sigmoid(z[:, 2 * H:3 * H] + dtype(O.FORGET_BIAS)), _sigmoid(z[:, 3 * H:])
    cn = c * f + i * j
    tc = np.tanh(cn)
    hn = tc * o
    if not scales:
        return hn, cn
    A = np.abs(xh).dot(np.abs(K)) + np.abs(b)
    Ai, Aj, Af, Ao = A[:, :H], A[:, H:2 * H], A[:, 2 * H:3 * H] + O.FORGET_BIAS, A[:, 3 * H:]
    di, dj = i * (1 - i) * Ai + i, (1 - j * j) * Aj + np.abs(j)
    df, do = f * (1 - f) * Af + f, o * (1 - o) * Ao + o
    Sc = np.abs(c) * df + np.abs(j) * di + i * dj + np.abs(c * f) + np.abs(i * j)
    Sh = o * (1 - tc * tc) * Sc + np.abs(tc) * do + np.abs(hn)
    return hn, cn, Sh, Sc, z


def measure(got, ref, S):
    """-> err [..] = |got - ref| / S where S > 0; where S == 0 the element must be the exact zero (err inf if it is not).  No element
    is left out: the result has got's shape."""
    got, ref, S = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(S, np.float64)
    assert got.shape == ref.shape == S.shape, (got.shape, ref.shape, S.shape)
    err = np.empty(got.shape)
    pos = S > 0
    err[pos] = np.abs(got[pos] - ref[pos]) / S[pos]
    err[~pos] = np.where(got[~pos] == 0.0, 0.0, np.inf)
    err[~np.isfinite(got)] = np.inf
    return err


def _family(err, e32, n_zero):
    e32 = max(float(e32), U)
    worst = np.unravel_index(int(np.argmax(err)), err.shape)
    return dict(ratio=float(err[worst] / e32), e32=e32, where=tuple(int(i) for i in worst), fails=int((err > M * e32).sum()),
                n=int(err.size), n_zero=int(n_zero))


def check_cell(params, cfg, tok, h0, c0, h1, c1):
    """One step of every layer: h0, c0 fp32 [L, R, H] as set, tok [R] the pending tokens, h1, c1 [L, R, H] or the padded [L, R, Hp] as
    read back.  -> {'c': .., 'h': ..}: worst err / e32, e32, the worst element (layer, row, unit), elements over M * e32, elements
    compared, of which with exact zero; and 'z_std', the spread of the fp64 pre-activations of each layer."""
    d = O.model_dims(cfg)
    L, H = d['L'], d['H']
    h1, c1 = np.asarray(h1), np.asarray(c1)
    Lg, R, Hg = h1.shape
    assert Lg == L and Hg >= H and h0.shape == (L, R, H) and c1.shape == h1.shape
    err = {f: np.zeros((L, R, Hg)) for f in FAMILIES}
    e32 = {f: 0.0 for f in FAMILIES}
    z_std = []
    for l in range(L):
        x = params['embedding'][np.asarray(tok)] if l == 0 else h1[l - 1][:, :H]     # the device's own input, upcast
        hn, cn, Sh, Sc, z = layer_step(params, l, H, x, h0[l], c0[l], np.float64, scales=True)
        h32, c32 = layer_step(params, l, H, x, h0[l], c0[l], np.float32)
        assert h32.dtype == np.float32 and c32.dtype == np.float32
        z_std.append(float(z.std()))
        pad = np.zeros((R, Hg - H))
        for f, got, ref, S, r32 in (('h', h1[l], hn, Sh, h32), ('c', c1[l], cn, Sc, c32)):
            assert np.all(S > 0)
            err[f][l] = measure(got, np.concatenate([ref, pad], 1), np.concatenate([S, pad], 1))
            e32[f] = max(e32[f], float(measure(r32, ref, S).max()))
    out = {f: _family(err[f], e32[f], L * R * (Hg - H)) for f in FAMILIES}
    out['z_std'] = z_std
    return out


def lp_reference(params, h_top):
    """h_top fp32 [H] -> fp64 log-probs [V1], S [V1], p [V1], lse"""
    W, b = params['softmax_w'].astype(np.float64), params['softmax_b'].astype(np.float64)
    h = np.asarray(h_top, np.float64)
    z = h.dot(W) + b
    mx = z.max()
    lse = mx + np.log(np.exp(z - mx).sum())
    p = np.exp(z - lse)
    Z = np.abs(h).dot(np.abs(W)) + np.abs(b)
    return z - lse, Z + p.dot(Z) + abs(lse), p, lse


def lp_fp32(params, h_top):
    """the plain fp32 restatement: every operation in fp32"""
    z = np.asarray(h_top, np.float32).dot(params['softmax_w']) + params['softmax_b']
    mx = z.max()
    lse = mx + np.log(np.exp(z - mx).sum(dtype=np.float32))
    out = z - lse
    assert out.dtype == np.float32
    return out


def check_lp(params, h_top, got, cols=None):
    """got [n]: the log-probs of columns cols (every column when None) of the row of h_top, the top layer's new h as read back"""
    ref, S, p, lse = lp_reference(params, h_top)
    V1 = ref.size
    cols = np.arange(V1) if cols is None else np.asarray(cols)
    got = np.asarray(got)
    assert got.shape == cols.shape
    e32 = max(float(measure(lp_fp32(params, h_top), ref, S).max()), U)
    err = measure(got, ref[cols], S[cols])
    out = _family(err, e32, 0)
    out['where'] = (int(cols[out['where'][0]]),)
    if cols.size == V1 and np.array_equal(cols, np.arange(V1)):
        out['sum'] = float(np.exp(got.astype(np.float64)).sum())
        out['sum_bound'] = float(M * e32 * p.dot(S))
        out['sum_ok'] = bool(abs(out['sum'] - 1.0) <= out['sum_bound'])
    return out


def report(label, res):
    """one line per family: what the GPU tests print and tests/COMPONENTWISE_DECODE.md records"""
    for f in ('c', 'h', 'lp'):
        if f in res:
            r = res[f]
            print('%-28s %-2s worst %.2f x e32  e32 %.2e  at %s  (%d elements, %d exact zeros, %d over M)' %
                  (label, f, r['ratio'], r['e32'], r['where'], r['n'], r['n_zero'], r['fails']))
            if 'sum' in r:
                print('%-28s    sum exp(lp) - 1 = %+.2e  (bound %.2e)' % (label, r['sum'] - 1.0, r['sum_bound']))


def passed(res):
    return all(res[f]['fails'] == 0 and res[f].get('sum_ok', True) for f in ('c', 'h', 'lp') if f in res)


# ---------------------------------------------------------------------------------------------------------------- the stand-in
# The planted mistakes: name -> what it needs of the shape (see StandIn).
PLANTS = ('drop_last_k', 'skip_partial_chunk', 'row_tile_alias', 'bias_tile', 'lse_over_ldl', 'no_forget_bias', 'stale_x', 'pad_nonzero')
DROP_SLOT = 5


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


class StandIn(object):
    """fp32 arithmetic in the kernels' order on the padded layout.  gemv_segment: a K segment of n rows is 16 slots of m = n / 16
    consecutive k; wave w owns slots 4w .. 4w + 3 and adds, for s = 0 .. m - 1 (registers hold GEN_CH of them at a time), the MFMA's
    sum over its four slots of act[k] W[k], k = slot m + s (taken as a chain of fused multiply-adds in slot order); the x segment and
    the h segment of a cell go into the same accumulator; the four waves' partials are added in order, then the bias; the gates are
    fp32; the lse is max + (float)log(sum in double of expf(z - max)) over ncols columns.

    plant: one of PLANTS --
      drop_last_k         the last k of slot DROP_SLOT of the h segment (cells) and of the logits is dropped
      skip_partial_chunk  a partial register chunk behind a full one is skipped (m > GEN_CH, m % GEN_CH != 0)
      row_tile_alias      rows 16 .. 31 read the h of the row 16 above them (cells)
      bias_tile           the bias of the last column tile of the logits comes from 16 columns earlier
      lse_over_ldl        max and sum of the lse run over ldl = round_up(V1, 64) columns of a zero-filled buffer
      no_forget_bias      f = sigmoid(z_f)
      stale_x             layer l > 0 reads the old h of layer l - 1
      pad_nonzero         the last pad unit of every layer's new h is 1e-30
    """

    def __init__(self, params, cfg, Hp, plant=None):
        assert plant is None or plant in PLANTS
        d = O.model_dims(cfg)
        self.d, self.plant, self.Hp = d, plant, Hp
        H, L, V1 = d['H'], d['L'], d['V1']
        self.Ep = round_up(d['E'], 16)
        assert Hp % 16 == 0 and Hp >= H
        self.emb = np.zeros((V1, self.Ep), np.float32)
        self.emb[:, :d['E']] = params['embedding']
        self.Kx, self.Kh, self.b = [], [], []
        for l in range(L):
            in_r, in_p = (d['E'], self.Ep) if l == 0 else (H, Hp)
            K = params['kernel_%d' % l]
            kx, kh, b = np.zeros((in_p, 4, Hp), np.float32), np.zeros((Hp, 4, Hp), np.float32), np.zeros((4, Hp), np.float32)
            kx[:in_r, :, :H] = K[:in_r].reshape(in_r, 4, H)
            kh[:H, :, :H] = K[in_r:].reshape(H, 4, H)
            b[:, :H] = params['bias_%d' % l].reshape(4, H)
            self.Kx.append(kx.reshape(in_p, 4 * Hp)); self.Kh.append(kh.reshape(Hp, 4 * Hp)); self.b.append(b.reshape(4 * Hp))
        self.W = np.zeros((Hp, V1), np.float32)
        self.W[:H] = params['softmax_w']
        self.sb = params['softmax_b'].astype(np.float32)

    def applies(self, R=CELL_ROWS, lp=False):
        """whether the planted mistake changes anything the check of this shape looks at"""
        d, p = self.d, self.plant
        ms = [self.Ep // 16, self.Hp // 16]
        if lp:
            if p == 'drop_last_k':
                return True
            if p == 'skip_partial_chunk':
                return ms[1] > GEN_CH and ms[1] % GEN_CH != 0
            if p == 'bias_tile':
                return d['V1'] > 16
            if p == 'lse_over_ldl':
                return d['V1'] % 64 != 0
            return False
        return {'drop_last_k': True, 'skip_partial_chunk': any(m > GEN_CH and m % GEN_CH for m in ms), 'row_tile_alias': R > 16,
                'no_forget_bias': True, 'stale_x': d['L'] > 1, 'pad_nonzero': self.Hp > d['H']}.get(p, False)

    def _segment(self, acc, act, w, drop=False):
        n = w.shape[0]
        m = n // 16
        act64, w64 = act.astype(np.float64), w.astype(np.float64)
        for wave in range(4):
            a = acc[wave]
            for c0 in range(0, m, GEN_CH):
                if self.plant == 'skip_partial_chunk' and c0 > 0 and c0 + GEN_CH > m:
                    continue
                for s in range(c0, min(c0 + GEN_CH, m)):
                    for g in range(4):
                        slot = 4 * wave + g
                        if drop and self.plant == 'drop_last_k' and slot == DROP_SLOT and s == m - 1:
                            continue
                        k = slot * m + s
                        a = (a.astype(np.float64) + act64[:, k:k + 1] * w64[k]).astype(np.float32)
            acc[wave] = a

    def cell(self, tok, h, c):
        """h, c fp32 [L, R, H] or padded -> the new padded h, c [L, R, Hp]"""
        L, H, Hp = self.d['L'], self.d['H'], self.Hp
        R = h.shape[1]
        hp, cp = np.zeros((L, R, Hp), np.float32), np.zeros((L, R, Hp), np.float32)
        hp[:, :, :h.shape[2]], cp[:, :, :c.shape[2]] = h, c
        hn_all, cn_all = np.zeros_like(hp), np.zeros_like(cp)
        x = self.emb[np.asarray(tok)]
        one = np.float32(1)
        for l in range(L):
            acc = [np.zeros((R, 4 * Hp), np.float32) for _ in range(4)]
            self._segment(acc, x, self.Kx[l])
            act = hp[l].copy()
            if self.plant == 'row_tile_alias' and R > 16:
                act[16:32] = hp[l][0:min(16, R - 16)]
            self._segment(acc, act, self.Kh[l], drop=True)
            z = (((acc[0] + acc[1]) + acc[2]) + acc[3]) + self.b[l]
            assert z.dtype == np.float32
            z = z.reshape(R, 4, Hp)
            si, tj, so = _sigmoid(z[:, 0]), np.tanh(z[:, 1]), _sigmoid(z[:, 3])
            sf = _sigmoid(z[:, 2] if self.plant == 'no_forget_bias' else z[:, 2] + one)
            cn = cp[l] * sf + si * tj
            hn = np.tanh(cn) * so
            assert hn.dtype == np.float32 and cn.dtype == np.float32
            if self.plant == 'pad_nonzero' and Hp > H:
                hn[:, Hp - 1] = np.float32(1e-30)
            hn_all[l], cn_all[l] = hn, cn
            x = hp[l] if self.plant == 'stale_x' else hn
        return hn_all, cn_all

    def logprobs(self, h_top, cols=None):
        """h_top [H] or padded [Hp]: the log-probs of one row at columns cols (all of them when None)"""
        V1, Hp = self.d['V1'], self.Hp
        ldl = round_up(V1, 64)
        h = np.zeros((1, Hp), np.float32)
        h[0, :len(h_top)] = h_top
        acc = [np.zeros((1, V1), np.float32) for _ in range(4)]
        self._segment(acc, h, self.W, drop=True)
        bias = self.sb.copy()
        if self.plant == 'bias_tile' and V1 > 16:
            t0 = 16 * ((V1 - 1) // 16)
            bias[t0:] = self.sb[t0 - 16:V1 - 16]
        row = np.zeros(ldl, np.float32)
        row[:V1] = ((((acc[0] + acc[1]) + acc[2]) + acc[3]) + bias)[0]
        n = ldl if self.plant == 'lse_over_ldl' else V1
        mx = row[:n].max()
        se = np.exp(row[:n] - mx).astype(np.float64).sum()
        lse = mx + np.float32(np.log(se))
        out = row[:V1] - lse
        assert out.dtype == np.float32
        return out if cols is None else out[np.asarray(cols)]


# ---------------------------------------------------------------------------------------------------------------- the two older checks
def older_checks_see(plant, shape, steps=12, rows=5):
    """Whether the two checks the suite had would have seen a planted mistake, restated on the stand-in at a shape test_dstate.py's
    test_e5 runs (parameters three oracle train steps from their initial values, five rows, twelve positions from the fresh state):
    'norm': max|err| / max|ref| of h or c after the twelve positions exceeds 2e-5; 'margin': at some position the greedy token's
    log-prob is off by more than 1e-4, or its fp64 logit is more than 1e-4 below the fp64 maximum (gen_ref.check_margins).
    -> dict(applies, norm, margin, worst_norm, worst_margin)"""
    cfg = config(shape['embedding_size'], shape['hidden_size'], shape.get('n_layers', 1), shape['input_size'])
    cfg['max_len'] = steps
    d = O.model_dims(cfg)
    params = O.glorot_init(cfg, 1234)
    opt = O.new_opt_state(params)
    for sup, qry in O.synthetic_episodes(3, 2, 2, 2, steps, d['V1'] - 1, seed=7):
        O.train_step(params, opt, sup, qry, cfg)
    p32 = {k: v.astype(np.float32) for k, v in params.items()}
    Hp = round_up(d['H'], 64) if d['H'] == 200 else round_up(d['H'], 16)
    sim = StandIn(p32, cfg, Hp, plant)
    toks = np.random.RandomState(3).randint(0, d['V1'] - 1, size=(rows, steps)).astype(np.int32)
    inputs = np.concatenate([np.full((rows, 1), d['start'], np.int32), toks[:, :-1]], 1)
    L, H = d['L'], d['H']
    h, c = np.zeros((L, rows, Hp), np.float32), np.zeros((L, rows, Hp), np.float32)
    h64, c64 = np.zeros((L, rows, H)), np.zeros((L, rows, H))
    worst_margin = 0.0
    for t in range(steps):
        h, c = sim.cell(inputs[:, t], h, c)
        x = p32['embedding'][inputs[:, t]].astype(np.float64)
        for l in range(L):
            h64[l], c64[l] = layer_step(p32, l, H, x, h64[l], c64[l])
            x = h64[l]
        for r in range(rows):
            lp = sim.logprobs(h[-1, r]).astype(np.float64)
            ref, _, _, _ = lp_reference(p32, h64[-1, r])
            g = int(np.argmax(lp))
            worst_margin = max(worst_margin, abs(lp[g] - ref[g]), ref.max() - ref[g])
    worst_norm = max(np.abs(h[:, :, :H] - h64).max() / np.abs(h64).max(), np.abs(c[:, :, :H] - c64).max() / np.abs(c64).max())
    return dict(applies=sim.applies(R=rows) or sim.applies(lp=True), norm=bool(worst_norm > 2e-5), margin=bool(worst_margin > 1e-4),
                worst_norm=float(worst_norm), worst_margin=float(worst_margin))
