"""numpy fp64 restatement of a decode state (include/fsmg.h fsmg_dstate_*, DESIGN.md "Decode states"): h and c of every layer, the
pending token, the last `history` context tokens and the two counters, with feed, generate (the Philox position runs on from n_gen,
the penalty's window reaches back into the history), gather, and the plugin's condition / eval_conditioned on top of them.  Built
from gen_ref's cell step and Gumbel noise and filter_ref's penalty and draw."""
import numpy as np

import filter_ref as F
import gen_ref as R
from oracle import lstm_oracle as O


class State(object):
    def __init__(self, params, config, rows, history):
        if rows < 1 or history < 1:
            raise ValueError('rows and history must be >= 1')
        self.params, self.config = params, config
        self.d = O.model_dims(config)
        self.rows, self.history = int(rows), int(history)
        self.reset()

    def reset(self):
        H, L = self.d['H'], self.d['L']
        self.hs = [[np.zeros(H) for _ in range(L)] for _ in range(self.rows)]
        self.cs = [[np.zeros(H) for _ in range(L)] for _ in range(self.rows)]
        self.pending = [self.d['start']] * self.rows       # the implicit start word: pending, but not context
        self.ctx = [[] for _ in range(self.rows)]          # the last `history` context tokens, oldest first
        self.n_ctx = self.n_gen = 0

    def _read(self, r):
        """row r reads its pending token -> the V1 logits after it"""
        return R._cell_step(self.params, self.d['H'], self.d['L'], self.params['embedding'][self.pending[r]], self.hs[r], self.cs[r])

    def _push(self, r, w):
        self.pending[r] = int(w)
        self.ctx[r] = (self.ctx[r] + [int(w)])[-self.history:]

    def feed(self, tokens, logprobs=False):
        """tokens int [rows, n], ids in [0, input_size] -> log-probs [rows, n] or None"""
        tokens = np.asarray(tokens)
        if tokens.ndim != 2 or tokens.shape[0] != self.rows:
            raise ValueError('tokens must be [rows, n]')
        if tokens.size and (tokens.min() < 0 or tokens.max() > self.d['start']):
            raise ValueError('token id outside [0, input_size]')
        n = tokens.shape[1]
        lp = np.zeros((self.rows, n))
        for r in range(self.rows):
            for i in range(n):
                x = int(tokens[r, i])
                if logprobs:
                    z = self._read(r)
                    lp[r, i] = z[x] - R.logsumexp(z)
                else:
                    self._read(r)
                self._push(r, x)
        self.n_ctx += n
        return lp if logprobs else None

    def check_window(self, num, theta, window):
        """the window rule of fsmg_dstate_generate (a penalty that is on must find its whole window in the history)"""
        if F.neutral(theta=theta):
            return
        if window < 0 or window > self.history:
            raise ValueError('repeat_window must be in [1, history]')
        if window == 0 and self.n_ctx + num > self.history:
            raise ValueError('repeat_window 0 needs n_ctx + num <= history')

    def generate(self, num, temperature=1.0, top_k=0, seed=0, top_p=0.0, min_p=0.0, theta=1.0, window=0):
        """-> tokens int [rows, num], log-probs [rows, num]; the Philox counter of local position t is (v >> 2, n_gen + t, row, 0)"""
        self.check_window(num, theta, window)
        V1 = self.d['V1']
        toks = np.zeros((self.rows, num), np.int64)
        lps = np.zeros((self.rows, num))
        plain = F.neutral(top_p, min_p, theta)
        for r in range(self.rows):
            for t in range(num):
                z = self._read(r)
                noise = R.gumbel(seed, self.n_gen + t, r, V1)
                if plain:
                    w, _ = R.choose(z, temperature, top_k, noise)
                else:
                    # the last min(window, n_ctx + t) tokens of (history followed by this call's tokens): ctx holds exactly those
                    zp = F.penalise(z, self.ctx[r], theta, window)
                    w, _, _ = F.choose(zp, temperature, top_k, top_p, min_p, noise)
                toks[r, t] = w
                lps[r, t] = z[w] - R.logsumexp(z)
                self._push(r, w)
        self.n_ctx += num
        self.n_gen += num
        return toks, lps

    def gather(self, src, rows):
        """this state's row i = src's row rows[i]; the counters are copied"""
        rows = [int(i) for i in rows]
        if src is self or src.history != self.history or len(rows) != self.rows or min(rows) < 0 or max(rows) >= src.rows:
            raise ValueError('bad gather')
        self.hs = [[v.copy() for v in src.hs[i]] for i in rows]
        self.cs = [[v.copy() for v in src.cs[i]] for i in rows]
        self.pending = [src.pending[i] for i in rows]
        self.ctx = [list(src.ctx[i]) for i in rows]
        self.n_ctx, self.n_gen = src.n_ctx, src.n_gen

    def arrays(self):
        """-> h, c [L, rows, H], ctx [rows, min(n_ctx, history)]: what fsmg_dstate_get returns"""
        L = self.d['L']
        h = np.stack([np.stack([self.hs[r][l] for r in range(self.rows)]) for l in range(L)])
        c = np.stack([np.stack([self.cs[r][l] for r in range(self.rows)]) for l in range(L)])
        return h, c, np.array(self.ctx, np.int64).reshape(self.rows, min(self.n_ctx, self.history))


def condition(params, config, support, history=None):
    """LSTMBaseline.condition: support int [A, K, T] -> a State of A rows that has read song_1, then [start] + song_k, k = 2..K"""
    support = np.asarray(support)
    A, K, T = support.shape
    st = State(params, config, A, history or K * (T + 1) + 2 * T)
    start = np.full((A, 1), st.d['start'], np.int64)
    for k in range(K):
        st.feed(support[:, k] if k == 0 else np.concatenate([start, support[:, k]], axis=1))
    return st


def eval_conditioned(params, config, support, query):
    """LSTMBaseline.eval_conditioned: the mean NLL of the query songs' tokens, each song read behind its artist's support songs"""
    query = np.asarray(query)
    N, Q, T = query.shape
    st = condition(params, config, support)
    rows = State(params, config, N * Q, st.history)
    rows.gather(st, np.repeat(np.arange(N), Q))
    start = np.full((N * Q, 1), st.d['start'], np.int64)
    lp = rows.feed(np.concatenate([start, query.reshape(N * Q, T)], axis=1), logprobs=True)
    return float(-np.mean(lp[:, 1:]))
