"""LSTM baseline with a support-set neural cache at evaluation time -- MI355X-native plugin.

The baseline's eval ignores each episode's support set.  CacheLSTM trains exactly like LSTMBaseline (train and sample are
inherited; generate too unless cache=True) and uses the support set at evaluation time without a gradient (Grave, Joulin, Usunier: Improving neural language
models with a continuous cache): the top-layer hidden states the model produced while reading an artist's support songs are
kept with the token that followed each (include/fsmg.h fsmg_cache_*); at every query position the model's own hidden state
attends over its artist's entries, and the resulting distribution is mixed with the model's:

    p(y) = (1 - cache_lambda) p_lstm(y) + cache_lambda p_cache(y),   p_cache = softmax(cache_theta q . k) mass on the entries holding y

Config keys beyond LSTMBaseline's: cache_theta (sharpness, >= 0) and cache_lambda (mixing weight in [0, 1]; 0 is the baseline).
Optional: cache_self (default false) adds every song's OWN history to the set it attends over -- the hidden states of its earlier
positions, each with the token that followed (include/fsmg.h fsmg_cache_self_*): one softmax over the union, the same theta and
lambda -- and cache_window (default max_len) is how many of its own last positions a position sees.  With cache_self unset every
path below is what it was, bit for bit.
Optional: cache_lengths (default false, and then every path is what it was) takes the songs' true lengths into evaluation
(include/fsmg.h "per-song lengths in scoring and in the support-set cache"): only the positions inside a support song are filed as
cache entries, only the positions inside a query song are scored, and the NLL is the mean over the scored positions -- the number
LSTMBaseline reports with mask_padding on, now with the support set used.  eval, eval_many and tune read Episode.support_len /
query_len (a missing one is a ValueError); score takes support_lengths= and lengths=, generate(cache=True) takes support_len=.
Training is LSTMBaseline's unmasked step either way: `mask_padding: true` stays refused.

  generate(..., cache=True)  LSTMBaseline.generate's rows drawn from the mixture: every generated token attends over ONE cache group
                       built from the whole support set (fsmg_cache_generate); the default (cache=False) is the baseline's generate
  eval(episode)        mean NLL of the query tokens under the mixture (one fsmg_cache_eval_step)
  eval_many(episodes)  one call per episode
  score(s, songs)      builds a one-group cache from the support set and scores the songs against it
  tune(episodes, thetas, lambdas)  the [n_theta][n_lambda] grid of mean NLLs, one device pass per episode for the whole grid
  score_self(songs)    the songs under the pure self-cache: no support set at all

With cache_self set, eval, score, tune and generate(cache=True) use the union; generate(self_cache=True) draws from the rows' own
history alone and needs no support set.
"""
import numpy as np

from models.lstm_baseline import LSTMBaseline


class CacheLSTM(LSTMBaseline):
    MASKS_PADDING = False        # training has no masked form here: `mask_padding: true` is refused at construction (cache_lengths is the evaluation-side key)
    _self = False               # the defaults of the optional keys: the own history stays out of the set
    _window = None              # None: max_len
    _lengths_on = False         # cache_lengths: the songs' true lengths in eval, tune, score and the generation cache

    def __init__(self, config):
        for key in ('cache_theta', 'cache_lambda'):
            if key not in config:
                raise RuntimeError('required config key "%s" not found' % key)
        self._theta, self._lambda = float(config['cache_theta']), float(config['cache_lambda'])
        if not (np.isfinite(self._theta) and self._theta >= 0.0):
            raise RuntimeError('cache_theta must be finite and >= 0, got %r' % config['cache_theta'])
        if not 0.0 <= self._lambda <= 1.0:
            raise RuntimeError('cache_lambda must lie in [0, 1], got %r' % config['cache_lambda'])
        self._self = bool(config.get('cache_self', False))
        if not isinstance(config.get('cache_lengths', False), (bool, np.bool_)):
            raise RuntimeError('cache_lengths must be true or false, got %r' % (config['cache_lengths'],))
        self._lengths_on = bool(config.get('cache_lengths', False))
        if 'cache_window' in config and int(config['cache_window']) < 1:
            raise RuntimeError('cache_window must be >= 1, got %r' % config['cache_window'])
        super(CacheLSTM, self).__init__(config)
        self._window = int(config.get('cache_window', self._time_steps))

    def _episode(self, episode):
        support, query = self._tokens(episode.support, 3), self._tokens(episode.query, 3)
        if support.shape[0] != query.shape[0]:
            raise ValueError('support %r and query %r differ in their number of artists' % (support.shape, query.shape))
        return support, query

    @staticmethod
    def _len_kw(lengths):
        """the engine's lengths= keyword only where there are lengths: without them every call is, argument for argument, what it was"""
        return {} if lengths is None else dict(lengths=lengths)

    def _episode_lengths(self, episode):
        """(support_len int32 [N, K], query_len int32 [N, Q]) of an episode when cache_lengths is on, else (None, None)"""
        if not self._lengths_on:
            return None, None
        out = []
        for name in ('support', 'query'):
            ln, tokens = getattr(episode, name + '_len', None), getattr(episode, name)
            if ln is None:
                raise ValueError('cache_lengths is on and the episode has no %s_len: lengths come from EpisodeSampler.gather '
                                 '(or Episode(support, query, support_len, query_len))' % name)
            ln = np.ascontiguousarray(ln, dtype=np.int32)
            if ln.shape != tuple(np.shape(tokens)[:2]):
                raise ValueError('%s_len %r does not match the length of %s %r' % (name, ln.shape, name, np.shape(tokens)))
            out.append(ln)
        return tuple(out)

    def eval(self, episode):
        self._require_init()
        support, query = self._episode(episode)
        sl, ql = self._episode_lengths(episode)
        if self._self:
            nll = float(self._grid(support, query, [self._theta], [self._lambda], sl, ql)[0, 0])
        elif sl is not None:
            nll = self._model.cache_eval_step(support, query, self._theta, self._lambda, support_len=sl, query_len=ql)
        else:
            nll = self._model.cache_eval_step(support, query, self._theta, self._lambda)
        self._log_scalar('Eval/Avg_NLL', nll, self._eval_calls)
        self._eval_calls += 1
        return nll

    def eval_many(self, episodes):
        return [self.eval(e) for e in episodes]

    def score(self, support_set, songs, thetas=None, lambdas=None, support_lengths=None, **kw):
        """Per-token statistics of the given songs (int32 [R, max_len]) under the mixture, every song attending over ONE cache
        group built from the whole support set (int32 [.., max_len]).  thetas / lambdas default to the configured pair; the result is
        FsmgModel.cache_score's dict ('logprob' [n_theta, n_lambda, R, T], 'row_nll' [n_theta, n_lambda, R], and on request
        cache_prob=True, lstm_logprob=True).  Keywords: FsmgModel.cache_score's.  With cache_lengths on, support_lengths= (one per
        support song) and lengths= (one per song) are required: a ragged cache, and only the positions inside a song are scored."""
        self._require_init()
        if self._lengths_on and (support_lengths is None or kw.get('lengths') is None):
            raise ValueError('cache_lengths is on: score needs support_lengths= and lengths=')
        if not self._lengths_on and (support_lengths is not None or kw.get('lengths') is not None):
            raise ValueError('lengths were given and cache_lengths is off')
        cache = self._model.cache_build(support_set, n_groups=1, **self._len_kw(support_lengths))
        thetas, lambdas = self._theta if thetas is None else thetas, self._lambda if lambdas is None else lambdas
        try:
            if self._self:
                return self._model.cache_self_score(songs, thetas, lambdas, self._window, cache=cache, **kw)
            return self._model.cache_score(cache, songs, thetas, lambdas, **kw)
        finally:
            cache.close()

    def score_self(self, songs, thetas=None, lambdas=None, window=None, **kw):
        """score() without a support set: every song attends over its own history alone (its last `window` positions; default the
        configured cache_window).  Works whether or not cache_self is set.  Position 0, which has no history, is scored by the model.
        With cache_lengths on, lengths= (one per song) is required."""
        if self._lengths_on and kw.get('lengths') is None:
            raise ValueError('cache_lengths is on: score_self needs lengths=')
        self._require_init()
        return self._model.cache_self_score(songs, self._theta if thetas is None else thetas, self._lambda if lambdas is None else lambdas,
                                            self._window if window is None else window, **kw)

    def _own_window(self):
        return self._time_steps if self._window is None else self._window

    def _grid(self, support, query, thetas, lambdas, support_len=None, query_len=None):
        """float64 [n_theta, n_lambda]: one episode's mean query NLL at every pair, artist a's songs over artist a's entries; with
        lengths (cache_lengths) a ragged cache and the mean over the scored positions"""
        N, Q, T = query.shape
        kw = self._len_kw(query_len)
        cache = self._model.cache_build(support, n_groups=N, **self._len_kw(support_len))
        try:
            group = np.repeat(np.arange(N), Q)
            if self._self:
                lp = self._model.cache_self_score(query, thetas, lambdas, self._window, cache=cache, group=group, row_nll=False, **kw)['logprob']
            else:
                lp = self._model.cache_score(cache, query, thetas, lambdas, group=group, row_nll=False, **kw)['logprob']
        finally:
            cache.close()
        if query_len is None:
            return -lp.astype(np.float64).mean(axis=(2, 3))
        return -lp.astype(np.float64).sum(axis=(2, 3)) / float(np.sum(query_len))        # the unscored positions are exact zeros

    def generate(self, support_set, num, n=1, cache=False, self_cache=False, support_len=None, **kw):
        """LSTMBaseline.generate (its keywords; cache=False and self_cache=False: exactly it).  cache=True: a one-group cache is
        built from the whole support set (int32 [.., max_len]), every generated token is drawn from the mixture at the configured
        cache_theta and cache_lambda, and the cache is closed; with the config's cache_self set the rows' own history (the last
        cache_window positions, primer included) joins the set, as in eval, score and tune.  self_cache=True: the own history is in
        the set whatever the config says, and with cache=False it is the whole set -- the support set may then be empty (primer_len
        0).  The union has no decode-state variant: condition_on_support=True is refused with it.  With cache=True and no self-cache,
        condition_on_support=True also starts the rows from a decode state primed on the support songs.  The log-probs
        (logprobs=True) are the mixture's.  With cache_lengths on, cache=True needs support_len= (one length per support song): the
        cache holds only the positions inside each song."""
        if cache and self._lengths_on and support_len is None:
            raise ValueError('cache_lengths is on: generate(cache=True) needs support_len=')
        if support_len is not None and not (cache and self._lengths_on):
            raise ValueError('support_len goes with cache=True and cache_lengths: true')
        if not cache and not self_cache:
            return super(CacheLSTM, self).generate(support_set, num, n=n, **kw)
        self._require_init()
        own = self_cache or self._self
        if own and kw.get('condition_on_support'):
            raise ValueError('the self-cache has no decode-state variant: condition_on_support=True cannot be combined with it')
        songs = np.ascontiguousarray(support_set, dtype=np.int32).reshape(-1, self._time_steps)
        built = self._model.cache_build(songs, n_groups=1, **self._len_kw(support_len)) if cache else None
        if own:
            draw = lambda n_seq, count, **g: self._model.cache_self_generate(n_seq, count, self._theta, self._lambda, self._own_window(),
                                                                             cache=built, **g)
        else:
            draw = lambda n_seq, count, **g: self._model.cache_generate(built, n_seq, count, self._theta, self._lambda, **g)
        try:
            return super(CacheLSTM, self).generate(support_set, num, n=n, _draw=draw, **kw)
        finally:
            if built is not None:
                built.close()

    def tune(self, episodes, thetas, lambdas):
        """float64 [n_theta, n_lambda]: the mean over the episodes of the query NLL at every (theta, lambda) -- what eval would
        return with that pair configured.  One cache build and one scoring pass per episode for the whole grid."""
        self._require_init()
        total, count = None, 0
        for e in episodes:
            support, query = self._episode(e)
            nll = self._grid(support, query, thetas, lambdas, *self._episode_lengths(e))
            total = nll if total is None else total + nll
            count += 1
        if count == 0:
            raise ValueError('tune needs at least one episode')
        return total / count
