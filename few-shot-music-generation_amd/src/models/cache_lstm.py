"""LSTM baseline with a support-set neural cache at evaluation time -- MI355X-native plugin.

The baseline's eval ignores each episode's support set.  CacheLSTM trains exactly like LSTMBaseline (train and sample are
inherited; generate too unless cache=True) and uses the support set at evaluation time without a gradient (Grave, Joulin, Usunier: Improving neural language
models with a continuous cache): the top-layer hidden states the model produced while reading an artist's support songs are
kept with the token that followed each (include/fsmg.h fsmg_cache_*); at every query position the model's own hidden state
attends over its artist's entries, and the resulting distribution is mixed with the model's:

    p(y) = (1 - cache_lambda) p_lstm(y) + cache_lambda p_cache(y),   p_cache = softmax(cache_theta q . k) mass on the entries holding y

Config keys beyond LSTMBaseline's: cache_theta (sharpness, >= 0) and cache_lambda (mixing weight in [0, 1]; 0 is the baseline).

  generate(..., cache=True)  LSTMBaseline.generate's rows drawn from the mixture: every generated token attends over ONE cache group
                       built from the whole support set (fsmg_cache_generate); the default (cache=False) is the baseline's generate
  eval(episode)        mean NLL of the query tokens under the mixture (one fsmg_cache_eval_step)
  eval_many(episodes)  one call per episode
  score(s, songs)      builds a one-group cache from the support set and scores the songs against it
  tune(episodes, thetas, lambdas)  the [n_theta][n_lambda] grid of mean NLLs, one device pass per episode for the whole grid
"""
import numpy as np

from models.lstm_baseline import LSTMBaseline


class CacheLSTM(LSTMBaseline):
    def __init__(self, config):
        for key in ('cache_theta', 'cache_lambda'):
            if key not in config:
                raise RuntimeError('required config key "%s" not found' % key)
        self._theta, self._lambda = float(config['cache_theta']), float(config['cache_lambda'])
        if not (np.isfinite(self._theta) and self._theta >= 0.0):
            raise RuntimeError('cache_theta must be finite and >= 0, got %r' % config['cache_theta'])
        if not 0.0 <= self._lambda <= 1.0:
            raise RuntimeError('cache_lambda must lie in [0, 1], got %r' % config['cache_lambda'])
        super(CacheLSTM, self).__init__(config)

    def _episode(self, episode):
        support, query = self._tokens(episode.support, 3), self._tokens(episode.query, 3)
        if support.shape[0] != query.shape[0]:
            raise ValueError('support %r and query %r differ in their number of artists' % (support.shape, query.shape))
        return support, query

    def eval(self, episode):
        self._require_init()
        support, query = self._episode(episode)
        nll = self._model.cache_eval_step(support, query, self._theta, self._lambda)
        self._log_scalar('Eval/Avg_NLL', nll, self._eval_calls)
        self._eval_calls += 1
        return nll

    def eval_many(self, episodes):
        return [self.eval(e) for e in episodes]

    def score(self, support_set, songs, thetas=None, lambdas=None, **kw):
        """Per-token statistics of the given songs (int32 [R, max_len]) under the mixture, every song attending over ONE cache
        group built from the whole support set (int32 [.., max_len]).  thetas / lambdas default to the configured pair; the result is
        FsmgModel.cache_score's dict ('logprob' [n_theta, n_lambda, R, T], 'row_nll' [n_theta, n_lambda, R], and on request
        cache_prob=True, lstm_logprob=True).  Keywords: FsmgModel.cache_score's."""
        self._require_init()
        cache = self._model.cache_build(support_set, n_groups=1)
        try:
            return self._model.cache_score(cache, songs, self._theta if thetas is None else thetas,
                                           self._lambda if lambdas is None else lambdas, **kw)
        finally:
            cache.close()

    def generate(self, support_set, num, n=1, cache=False, **kw):
        """LSTMBaseline.generate (its keywords; cache=False: exactly it).  cache=True: a one-group cache is built from the whole
        support set (int32 [.., max_len]), every generated token is drawn from the mixture at the configured cache_theta and
        cache_lambda, and the cache is closed.  With condition_on_support=True the rows also start from a decode state primed on the
        support songs.  The log-probs (logprobs=True) are the mixture's."""
        if not cache:
            return super(CacheLSTM, self).generate(support_set, num, n=n, **kw)
        self._require_init()
        songs = np.ascontiguousarray(support_set, dtype=np.int32).reshape(-1, self._time_steps)
        built = self._model.cache_build(songs, n_groups=1)
        try:
            return super(CacheLSTM, self).generate(
                support_set, num, n=n, _draw=lambda n_seq, count, **g: self._model.cache_generate(built, n_seq, count, self._theta,
                                                                                               self._lambda, **g), **kw)
        finally:
            built.close()

    def tune(self, episodes, thetas, lambdas):
        """float64 [n_theta, n_lambda]: the mean over the episodes of the query NLL at every (theta, lambda) -- what eval would
        return with that pair configured.  One cache build and one scoring pass per episode for the whole grid."""
        self._require_init()
        total, count = None, 0
        for e in episodes:
            support, query = self._episode(e)
            N, Q, T = query.shape
            cache = self._model.cache_build(support, n_groups=N)
            try:
                lp = self._model.cache_score(cache, query, thetas, lambdas, group=np.repeat(np.arange(N), Q), row_nll=False)['logprob']
            finally:
                cache.close()
            nll = -lp.astype(np.float64).mean(axis=(2, 3))
            total = nll if total is None else total + nll
            count += 1
        if count == 0:
            raise ValueError('tune needs at least one episode')
        return total / count
