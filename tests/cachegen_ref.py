"""fp64 numpy restatement of cache-conditioned generation (include/fsmg.h "cache-conditioned generation"): the whole mixed
next-token distribution of a row, the free-running decoder that draws from it, and the teacher-forced margin check the GPU tests use.

    distribution   d_i = q . k_i over the row's group;  w_i = exp(theta (d_i - d_max));  p_cache(v) = sum_{i : v_i = v} w_i / sum_i w_i,
                   exactly 0 for a column no entry holds;  lp = z - logsumexp(z);  z'' = cache_ref.mix64(lp, p_cache, lambda)
    generate       gen_ref.generate with the mix step between the logits and the pick: the pick reads z'' as if it were the logits row
    check_margins  gen_ref.check_margins on the mixed rows, with a tolerance per position

dtype = np.float32 evaluates p_cache's formulas in fp32 (the GPU tests' tolerance is derived from its error).

oracle_case(name) is the input set the teacher-forced GPU test and the CPU test of its near-tie share have in common."""
import functools

import numpy as np

import cache_ref as C
import gen_ref as G
from conftest import small_config
from oracle import lstm_oracle as O


def cache_prob(keys, vals, q, theta, V1, dtype=np.float64):
    """one group: keys [Mg, H], vals [Mg], q [n, H] -> p_cache [n, V1] in dtype, exactly 0 in the columns no entry holds"""
    keys, q = np.asarray(keys, dtype), np.asarray(q, dtype)
    vals = np.asarray(vals).astype(np.int64)
    d = q.dot(keys.T)                                            # [n, Mg]
    w = np.exp(dtype(theta) * (d - d.max(axis=1, keepdims=True)))
    held, inv = np.unique(vals, return_inverse=True)
    onehot = np.zeros((vals.size, held.size), dtype)
    onehot[np.arange(vals.size), inv] = 1
    out = np.zeros((q.shape[0], V1), dtype)
    out[:, held] = w.dot(onehot) / w.sum(axis=1, dtype=dtype, keepdims=True)
    return out


def distribution(keys, vals, q, z, group, theta, lam, dtype=np.float64):
    """keys [G, Mg, H], vals [G, Mg], q [n, H], logits z [n, V1], group [n] (None: all 0) -> dict: cache_prob [n, V1] in dtype,
    lse [n], lp [n, V1] and logprob [n, V1] (z'', not rounded) in fp64"""
    q, z = np.asarray(q), np.asarray(z, np.float64)
    n, V1 = z.shape
    group = np.zeros(n, np.int64) if group is None else np.asarray(group).astype(np.int64)
    pc = np.zeros((n, V1), dtype)
    for g in np.unique(group):
        sel = np.flatnonzero(group == g)
        pc[sel] = cache_prob(keys[g], vals[g], q[sel], theta, V1, dtype)
    lse = np.array([G.logsumexp(row) for row in z])
    lp = z - lse[:, None]
    return dict(cache_prob=pc, lse=lse, lp=lp, logprob=C.mix64(lp, pc, lam))


def l1_of(q, keys_g):
    """what the project's per-unit hidden-state bound multiplies in a score of this query: sum_j |q_j| + max_i sum_j |k_ij|"""
    return float(np.abs(q).sum() + np.abs(keys_g).sum(axis=1).max())


def tolerance(theta, l1):
    """test_score_against_the_fp64_oracle's bound on a mixed log-prob: 1e-4 for the model's own, 2e-5 per hidden unit in theta d"""
    return 1e-4 + theta * 2e-5 * l1


def _margin(score):
    srt = np.sort(score[np.isfinite(score)])
    return float(srt[-1] - srt[-2]) if srt.size > 1 else np.inf


def _mixed_rows(params, config, inputs, keys_g, vals_g, theta, lam):
    """one row teacher-forced over `inputs`: -> z'' [len(inputs), V1] (fp64) and the tolerance of each position"""
    d = O.model_dims(config)
    H, L = d['H'], d['L']
    hs = [np.zeros(H) for _ in range(L)]
    cs = [np.zeros(H) for _ in range(L)]
    rows, tols = [], []
    for w in inputs:
        lg = G._cell_step(params, H, L, params['embedding'][w], hs, cs)
        q = hs[L - 1]
        pc = cache_prob(keys_g, vals_g, q[None], theta, d['V1'])[0]
        rows.append(C.mix64(lg - G.logsumexp(lg), pc, lam))
        tols.append(tolerance(theta, l1_of(q, keys_g)))
    return np.stack(rows), np.array(tols)


def generate(params, config, keys, vals, group, theta, lam, n_seq, num, temperature=1.0, top_k=0, seed=0, primer=None):
    """the free-running fp64 draw from the mixture -> dict: toks int [B, num], lps [B, num], margin [B, num] (the fp64 margin of each
    pick), tol [B, num] (tolerance() of each position)"""
    d = O.model_dims(config)
    H, L = d['H'], d['L']
    P = 0 if primer is None else np.asarray(primer).shape[1]
    group = np.zeros(n_seq, np.int64) if group is None else np.asarray(group)
    out = dict(toks=np.zeros((n_seq, num), np.int64), lps=np.zeros((n_seq, num)), margin=np.zeros((n_seq, num)), tol=np.zeros((n_seq, num)))
    for b in range(n_seq):
        kg, vg = np.asarray(keys[group[b]], np.float64), vals[group[b]]
        hs = [np.zeros(H) for _ in range(L)]
        cs = [np.zeros(H) for _ in range(L)]
        inputs = [d['start']] + ([] if P == 0 else [int(w) for w in primer[b]])
        for w in inputs[:-1]:
            G._cell_step(params, H, L, params['embedding'][w], hs, cs)
        w = inputs[-1]
        for t in range(num):
            lg = G._cell_step(params, H, L, params['embedding'][w], hs, cs)
            q = hs[L - 1]
            zz = C.mix64(lg - G.logsumexp(lg), cache_prob(kg, vg, q[None], theta, d['V1'])[0], lam)
            w, score = G.choose(zz, temperature, top_k, G.gumbel(seed, t, b, d['V1']))
            out['toks'][b, t], out['lps'][b, t] = w, zz[w] - G.logsumexp(zz)
            out['margin'][b, t], out['tol'][b, t] = _margin(score), tolerance(theta, l1_of(q, kg))
    return out


def check_margins(params, config, keys, vals, group, theta, lam, toks, lps, temperature, top_k, seed, primer=None, rows=None,
                  tokens=True):
    """gen_ref.check_margins on mixed rows.  Row b's own token history is fed into the fp64 decoder; at every generated position,
    with tol = tolerance() there: the GPU log-prob is within tol of z''_tok - logsumexp(z''), and (tokens=True) the GPU token's
    perturbed score is within tol of the fp64 maximum, lies in the fp64 top-k set (threshold tolerance tol: the row it is read from
    carries that error), and is the fp64 choice wherever the fp64 margin is >= 2 tol.
    -> dict: near (near-ties seen), total, lp_err (largest log-prob error), lp_tol (tol there), slack (largest shortfall of a
    perturbed score against the fp64 maximum), tol_min, tol_max"""
    d = O.model_dims(config)
    B, num = toks.shape
    P = 0 if primer is None else np.asarray(primer).shape[1]
    group = np.zeros(B, np.int64) if group is None else np.asarray(group)
    res = dict(near=0, total=0, lp_err=0.0, lp_tol=0.0, slack=0.0, tol_min=np.inf, tol_max=0.0)
    for b in (range(B) if rows is None else rows):
        inputs = [d['start']] + ([] if P == 0 else [int(w) for w in primer[b]]) + [int(w) for w in toks[b, :-1]]
        zz_all, tol_all = _mixed_rows(params, config, inputs, np.asarray(keys[group[b]], np.float64), vals[group[b]], theta, lam)
        zz_all, tol_all = zz_all[P:], tol_all[P:]
        for t in range(num):
            zz, tol, g = zz_all[t], float(tol_all[t]), int(toks[b, t])
            assert 0 <= g < d['V1'], (b, t, g)
            res['total'] += 1
            res['tol_min'], res['tol_max'] = min(res['tol_min'], tol), max(res['tol_max'], tol)
            want_lp = zz[g] - G.logsumexp(zz)
            assert np.isfinite(want_lp), ('a token the fp64 mixture gives no mass', b, t, g)
            e = abs(float(lps[b, t]) - want_lp)
            if e > res['lp_err']:
                res['lp_err'], res['lp_tol'] = e, tol
            assert e <= tol, ('logprob', b, t, lps[b, t], want_lp, tol)
            if not tokens:
                continue
            noise = G.gumbel(seed, t, b, d['V1'])
            want, score = G.choose(zz, temperature, top_k, noise)
            if top_k not in (0, d['V1']):
                thr = np.sort(zz)[::-1][top_k - 1]
                assert zz[g] >= thr - tol, ('outside top-k', b, t, g, zz[g], thr)
            sg = zz[g] if temperature == 0 or top_k == 1 else zz[g] / temperature + noise[g]
            res['slack'] = max(res['slack'], float(score[want] - sg))
            assert sg >= score[want] - tol, ('margin', b, t, g, want, sg, score[want], tol)
            if _margin(score) >= 2 * tol:
                assert g == want, ('token', b, t, g, want, _margin(score), tol)
            else:
                res['near'] += 1
    return res


# ------------------------------------------------------------------------------------------------ the teacher-forced test's inputs
SHAPES = {
    'H24': dict(input_size=300, max_len=16, embedding_size=20, hidden_size=24, n_layers=1),
    'H200x2': dict(input_size=300, max_len=16, embedding_size=20, hidden_size=200, n_layers=2),
    'H512': dict(input_size=300, max_len=16, embedding_size=20, hidden_size=512, n_layers=1),
}
GROUP = np.array([0, 0, 1, 1, 0], np.int32)         # 5 rows over 2 groups
NUM = 12
LAMBDA = 0.25
PICKS = ((1.0, 0), (1.0, 5), (0.7, 5))              # (temperature, top_k)
SEED = 21


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    """-> dict: cfg; params (fp64: the oracle's initialiser and three of its train steps, as test_cache's shapes); support [6, T] in 2
    groups x 3 songs; keys float32 [2, 3 T, H] (cache_ref.oracle_hidden of the support rows, rounded to what a cache stores), vals
    [2, 3 T]; primer [5, 3] (each row continues the head of a support song of its own group); thetas: fp32 numbers with theta *
    dmax = 0.3, 5, 40, dmax the largest |k_i . k_j| inside a group -- the support rows' own hidden states stand in for the queries,
    which are not known before the rows are drawn"""
    cfg = small_config(**SHAPES[name])
    params = O.glorot_init(cfg, cfg['seed'])
    opt = O.new_opt_state(params)
    for sup, qry in O.synthetic_episodes(3, 2, 2, 2, cfg['max_len'], cfg['input_size'], seed=7):
        O.train_step(params, opt, sup, qry, cfg)
    params = {k: np.asarray(v, np.float32).astype(np.float64) for k, v in params.items()}       # what a handle holds
    support = np.random.RandomState(11).randint(0, cfg['input_size'], size=(6, cfg['max_len'])).astype(np.int32)
    hs, _ = C.oracle_hidden(params, support, cfg)
    keys, vals = C.entries(hs, support, 2)
    keys = keys.astype(np.float32)
    k64 = keys.astype(np.float64)
    dmax = max(float(np.abs(k64[g].dot(k64[g].T)).max()) for g in range(2))
    thetas = [float(np.float32(x / dmax)) for x in (0.3, 5.0, 40.0)]
    primer = np.stack([support[3 * GROUP[b] + b % 3, :3] for b in range(5)]).astype(np.int32)
    return dict(cfg=cfg, params=params, support=support, keys=keys, vals=vals.astype(np.int32), primer=primer, thetas=thetas)
