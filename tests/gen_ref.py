"""numpy restatement of fsmg_generate (include/fsmg.h, DESIGN.md "Batched generation"): Philox4x32-10, Gumbel noise, the fp64
reference decoder built from oracle.lstm_oracle pieces, and the teacher-forced margin check the GPU tests use."""
import numpy as np

from oracle import lstm_oracle as O

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: uint32 [..., 4], key: (k0, k1) -> uint32 [..., 4]"""
    c = [np.asarray(ctr, np.uint64)[..., i] for i in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, -1).astype(np.uint32)


def gumbel(seed, t, b, V1):
    """Gumbel noise of generated token t of row b over the V1 columns (fp64)"""
    q = np.arange((V1 + 3) // 4, dtype=np.uint64)
    ctr = np.stack([q, np.full_like(q, t), np.full_like(q, b), np.zeros_like(q)], -1)
    x = philox4x32_10(ctr, (int(seed) & 0xFFFFFFFF, int(seed) >> 32)).reshape(-1)[:V1]
    u = ((x >> 8).astype(np.float64) + 0.5) * 2.0 ** -24
    return -np.log(-np.log(u))


def _cell_step(params, H, L, x, hs, cs):
    for l in range(L):
        z = np.concatenate([x, hs[l]]).dot(params['kernel_%d' % l]) + params['bias_%d' % l]
        i, j, f, o = z[:H], z[H:2 * H], z[2 * H:3 * H], z[3 * H:]
        cs[l] = cs[l] * O._sigmoid(f + O.FORGET_BIAS) + O._sigmoid(i) * np.tanh(j)
        hs[l] = np.tanh(cs[l]) * O._sigmoid(o)
        x = hs[l]
    return x.dot(params['softmax_w']) + params['softmax_b']


def row_logits(params, config, inputs):
    """fp64 logits after each input token of one row: [len(inputs), V1]"""
    d = O.model_dims(config)
    H, L = d['H'], d['L']
    hs = [np.zeros(H) for _ in range(L)]
    cs = [np.zeros(H) for _ in range(L)]
    return np.stack([_cell_step(params, H, L, params['embedding'][w], hs, cs) for w in inputs])


def allowed(logits, top_k):
    V1 = logits.shape[-1]
    if top_k in (0, V1):
        return np.ones(V1, bool)
    thr = np.sort(logits)[::-1][top_k - 1]
    return logits >= thr


def choose(logits, temperature, top_k, noise):
    """-> (token, perturbed scores over the allowed set (-inf elsewhere))"""
    if temperature == 0 or top_k == 1:
        return int(np.argmax(logits)), logits.copy()
    score = np.where(allowed(logits, top_k), logits / temperature + noise, -np.inf)
    return int(np.argmax(score)), score


def logsumexp(x):
    m = np.max(x)
    return m + np.log(np.sum(np.exp(x - m)))


def generate(params, config, n_seq, num, temperature=1.0, top_k=0, seed=0, primer=None):
    """the free-running fp64 draw: -> tokens int [B, num], log-probs [B, num]"""
    d = O.model_dims(config)
    P = 0 if primer is None else np.asarray(primer).shape[1]
    toks = np.zeros((n_seq, num), np.int64)
    lps = np.zeros((n_seq, num))
    for b in range(n_seq):
        H, L = d['H'], d['L']
        hs = [np.zeros(H) for _ in range(L)]
        cs = [np.zeros(H) for _ in range(L)]
        inputs = [d['start']] + ([] if P == 0 else [int(w) for w in primer[b]])
        for w in inputs[:-1]:
            _cell_step(params, H, L, params['embedding'][w], hs, cs)
        w = inputs[-1]
        for t in range(num):
            lg = _cell_step(params, H, L, params['embedding'][w], hs, cs)
            w, _ = choose(lg, temperature, top_k, gumbel(seed, t, b, d['V1']))
            toks[b, t] = w
            lps[b, t] = lg[w] - logsumexp(lg)
    return toks, lps


def check_margins(params, config, toks, lps, temperature, top_k, seed, primer=None, rows=None, tol=1e-4, tie=1e-4):
    """Teacher-forced check of GPU output: feed row b's own token history into the fp64 decoder; at every generated position the
    GPU token's perturbed score is within tol of the fp64 maximum, lies in the fp64 top-k set (threshold tolerance 1e-5), its
    log-prob is within tol, and it equals the fp64 choice wherever the fp64 margin is >= tie.  -> number of near-ties seen."""
    d = O.model_dims(config)
    B, num = toks.shape
    P = 0 if primer is None else np.asarray(primer).shape[1]
    near = 0
    for b in (range(B) if rows is None else rows):
        inputs = [d['start']] + ([] if P == 0 else [int(w) for w in primer[b]]) + [int(w) for w in toks[b, :-1]]
        lg_all = row_logits(params, config, inputs)[P:]
        for t in range(num):
            lg, g = lg_all[t], int(toks[b, t])
            assert 0 <= g < d['V1'], (b, t, g)
            want, score = choose(lg, temperature, top_k, gumbel(seed, t, b, d['V1']))
            if top_k not in (0, d['V1']):
                thr = np.sort(lg)[::-1][top_k - 1]
                assert lg[g] >= thr - 1e-5, ('outside top-k', b, t, g, lg[g], thr)
            if temperature == 0 or top_k == 1:
                sg = lg[g]
            else:
                sg = lg[g] / temperature + gumbel(seed, t, b, d['V1'])[g]
            best = score[want]
            assert sg >= best - tol, ('margin', b, t, g, want, sg, best)
            assert abs(float(lps[b, t]) - (lg[g] - logsumexp(lg))) <= tol, ('logprob', b, t, lps[b, t], lg[g] - logsumexp(lg))
            srt = np.sort(score[np.isfinite(score)])
            margin = srt[-1] - srt[-2] if srt.size > 1 else np.inf
            if margin >= tie:
                assert g == want, ('token', b, t, g, want, margin)
            else:
                near += 1
    return near
