"""Dynamic evaluation of the LSTM baseline (Krause et al., arXiv 1709.07432; the second "adaptive language model" of the
reference's READING_LIST.md beside the continuous cache, models/cache_lstm.py) -- MI355X-native plugin.

Training is the baseline's, unchanged (train.train runs it).  Evaluation adapts: while the model reads an artist's songs it takes
a small gradient step on every segment it has just scored, pulled back towards the trained parameters by a decay term and, under the
'rms' rule, scaled per parameter by gradient statistics collected once on training data (collect_stats).  An episode is streamed
artist by artist, the K support songs and then the Q query songs; every query position is scored before the model has adapted on
it, and the trained parameters come back after every call (semantics in full: include/fsmg.h "dynamic evaluation").

  eval(episode) / eval_many   the NLL over all artists' scored query positions (fsmg_dyneval_eval_step)
  collect_stats(episodes)     forward + backward per episode at the trained parameters, ms_sum += g * g each
  score(support, songs, ...)  the stream support-then-songs of ONE artist: per-token log-probs and per-song NLLs of `songs`
  generate(support, num, ...) samples drawn at the parameters adapted on the support stream (fsmg_dyneval_generate)

Config keys (config/dyneval_lstm.yaml): dyneval_rule ('sgd' / 'rms'), dyneval_lr, dyneval_decay, dyneval_eps, dyneval_seg_len,
dyneval_rows_per_step, dyneval_clip (0: none), dyneval_adapt_query (adapt on the query songs too, after scoring them),
dyneval_lengths (per-song lengths from Episode.support_len / query_len; without it every song has max_len positions).
The statistics are saved and restored next to the native checkpoint (<name>.dyneval_stats.npz).
"""
import os

import numpy as np

from models.lstm_baseline import LSTMBaseline

DEFAULTS = dict(dyneval_rule='sgd', dyneval_lr=1e-2, dyneval_decay=0.0, dyneval_eps=1e-3, dyneval_seg_len=None,
                dyneval_rows_per_step=1, dyneval_clip=0.0, dyneval_adapt_query=True, dyneval_lengths=False)


def dyneval_settings(config):
    """the dyneval_* keys of a model config -> the keyword arguments of FsmgModel.dyneval_config (dyneval_seg_len defaults to max_len)"""
    c = dict(DEFAULTS)
    c.update({k: config[k] for k in DEFAULTS if k in config and config[k] is not None})
    rule = str(c['dyneval_rule']).lower()
    if rule not in ('sgd', 'rms'):
        raise RuntimeError("dyneval_rule must be 'sgd' or 'rms', got %r" % (c['dyneval_rule'],))
    # (a segment longer than a song is the whole song: the library takes seg_len in [1, max_len])
    seg = int(config['max_len']) if c['dyneval_seg_len'] is None else min(int(c['dyneval_seg_len']), int(config['max_len']))
    return dict(rule=rule, seg_len=seg, rows_per_step=int(c['dyneval_rows_per_step']), lr=float(c['dyneval_lr']),
                decay=float(c['dyneval_decay']), eps=float(c['dyneval_eps']), clip_norm=float(c['dyneval_clip']),
                adapt_reported=bool(c['dyneval_adapt_query']))


def save_stats(engine, path):
    """the statistics of an engine (FsmgModel) -> one .npz: count and ms_sum/<parameter name>"""
    count, _ = engine.dyneval_stats_info()
    blob = {'count': np.int64(count)}
    for name in engine.param_shapes:
        blob['ms_sum/' + name] = engine.dyneval_stats_get(name)
    tmp = path + '.tmp.npz'
    np.savez(tmp, **blob)
    os.replace(tmp, path)


def load_stats(engine, path):
    """-> True when the file exists and every tensor matched (the statistics are then the file's), else False with nothing set"""
    if not os.path.isfile(path):
        return False
    with np.load(path) as blob:
        names = list(engine.param_shapes)
        if 'count' not in blob or any('ms_sum/' + n not in blob or blob['ms_sum/' + n].shape != engine._shape(n) for n in names):
            return False
        engine.dyneval_stats_reset()
        for n in names:
            engine.dyneval_stats_set(n, blob['ms_sum/' + n])
        engine.dyneval_stats_set_count(int(blob['count']))
    return True


class DynEvalLSTM(LSTMBaseline):
    MASKS_PADDING = False        # the baseline's one-pass masked loss is refused; this plugin's key is dyneval_lengths

    def __init__(self, config):
        super(DynEvalLSTM, self).__init__(config)
        self._dyn = dyneval_settings(config)
        self.dyneval_lengths = bool(config.get('dyneval_lengths', False))

    def _stats_path(self, checkpt_path):
        return os.path.join(checkpt_path, self.name, self.name + '.dyneval_stats.npz')

    def save(self, checkpt_path):
        super(DynEvalLSTM, self).save(checkpt_path)
        if self._model.dyneval_stats_info()[0] > 0:
            save_stats(self._model, self._stats_path(checkpt_path))

    def recover_or_init(self, init_path):
        super(DynEvalLSTM, self).recover_or_init(init_path)
        if init_path and load_stats(self._model, self._stats_path(init_path)):
            print('recovered the dynamic-evaluation statistics (%d passes)' % self._model.dyneval_stats_info()[0])

    def _episode_lengths(self, episode):
        if not self.dyneval_lengths:
            return None, None
        for name in ('support', 'query'):
            if getattr(episode, name + '_len', None) is None:
                raise ValueError('dyneval_lengths is on and the episode has no %s_len: lengths come from EpisodeSampler.gather '
                                 '(or Episode(support, query, support_len, query_len))' % name)
        return tuple(self._lengths(episode, ('support', 'query')))

    def collect_stats(self, episodes, reset=True):
        """one forward + backward per episode at the trained parameters (over the songs' own positions with dyneval_lengths), its
        squared gradient added to the statistics -> the number of accumulated passes"""
        self._require_init()
        if reset:
            self._model.dyneval_stats_reset()
        for e in episodes:
            sup, qry = self._tokens(e.support, 3), self._tokens(e.query, 3)
            sl, ql = self._episode_lengths(e)
            if sl is not None:
                self._model.forward_backward_masked(sup, qry, sl, ql)
            else:
                self._model.forward_backward(sup, qry)
            self._model.dyneval_stats_accumulate()
        return self._model.dyneval_stats_info()[0]

    def eval(self, episode):
        self._require_init()
        sl, ql = self._episode_lengths(episode)
        nll = self._model.dyneval_eval_step(self._dyn, self._tokens(episode.support, 3), self._tokens(episode.query, 3), sl, ql)
        self._log_scalar('Eval/Avg_NLL', nll, self._eval_calls)
        self._eval_calls += 1
        return nll

    def eval_many(self, episodes):
        """adaptation is per artist, so there is nothing to batch: one eval per episode"""
        return [self.eval(e) for e in episodes]

    def _support_stream(self, support_set, support_len):
        support = self._tokens(support_set, 2)
        if support_len is None:
            if self.dyneval_lengths:
                raise ValueError('dyneval_lengths is on: the support set needs its lengths (support_len=)')
            return support, None
        if not self.dyneval_lengths:
            raise ValueError('support_len needs dyneval_lengths: true in the model config')
        ln = np.ascontiguousarray(support_len, dtype=np.int32).reshape(-1)
        if ln.size != support.shape[0]:
            raise ValueError('support_len %r does not match the %d support songs' % (np.shape(support_len), support.shape[0]))
        return support, ln

    def score(self, support_set, songs, support_len=None, lengths=None):
        """the stream (support songs, then `songs`) of one artist -> dict(logprob [R, max_len], row_nll [R], nll) of `songs`, each
        position scored before the model has adapted on it; lengths: the scored songs' own (dyneval_lengths)"""
        self._require_init()
        support, sl = self._support_stream(support_set, support_len)
        songs = self._tokens(songs, 2)
        ln = None
        if self.dyneval_lengths:
            if lengths is None:
                raise ValueError('dyneval_lengths is on: the scored songs need their lengths (lengths=)')
            ln = np.concatenate([sl, np.ascontiguousarray(lengths, dtype=np.int32).reshape(-1)])
        elif lengths is not None:
            raise ValueError('lengths needs dyneval_lengths: true in the model config')
        k = support.shape[0]
        out = self._model.dyneval_score(self._dyn, np.concatenate([support, songs]), ln, first_reported=k)
        return dict(logprob=out['logprob'][k:], row_nll=out['row_nll'][k:], nll=out['nll'])

    def generate(self, support_set, num, n=1, temperature=1.0, top_k=0, seed=0, primer_len=0, logprobs=False, top_p=0.0, min_p=0.0,
                 repetition_penalty=1.0, repeat_window=0, support_len=None):
        """like LSTMBaseline.generate, at the parameters adapted on the support stream; the trained parameters are restored"""
        self._require_init()
        support, sl = self._support_stream(support_set, support_len)
        return self._model.dyneval_generate(self._dyn, support, int(num), support_len=sl, n_seq=int(n), temperature=temperature,
                                            top_k=top_k, seed=seed, primer=self._primer(support, int(n), int(primer_len)),
                                            logprobs=logprobs, top_p=top_p, min_p=min_p, repetition_penalty=repetition_penalty,
                                            repeat_window=repeat_window)
