"""MAML-style few-shot LSTM language model (BASELINE.json configs[4], "cfg-E") -- MI355X-native plugin.

The reference ships no meta-learning model; its READING_LIST.md:5-7 names MAML ("Model-agnostic meta-learning for fast
adaptation of deep networks") as the direction the project was heading.  This plugin keeps the models/ plugin API
(src/models/base_model.py:4-54) and the LSTM-baseline architecture and config keys, and changes what an episode means
(semantics in DESIGN.md "cfg-E"; CPU oracle oracle/lstm_oracle.py maml_step / maml_eval), first order:

  train(episode)  theta' = theta after `inner_steps` steps of clipped SGD (`inner_lr`) on the SUPPORT set; the gradient
                  of the QUERY set's mean NLL at theta' is applied to theta with the baseline's clip + Adam; returns the
                  query NLL at theta' (before the outer update).  Episode-parallel: the inner loop is per rank and needs no
                  communication, the query gradients are all-reduced exactly like a baseline step's.
  eval(episode)   adapt on the support set, mean NLL of the query set at theta', then theta is restored.
  sample(s, num)  greedy decode at theta (the support set is not used, as in the baseline).
  generate(s, num, n, ...)  n samples drawn at theta' adapted on the support set s (fsmg_maml_generate): generation AS the
                  episode's artist.
  beam_search(s, num, beam_width, n, ...)  the same at theta' (fsmg_maml_beam_search).
  score(s, songs, ...)  per-token log-probabilities, ranks, entropies and per-song NLLs of given songs at theta' adapted on the
                  support set s (fsmg_maml_score); theta is restored.

Extra config keys: inner_steps (default 1), inner_lr (default 0.1), maml_lengths (default false: every path is what it was;
true: per-song lengths, DESIGN.md 22 -- every inner step averages over the positions inside a support song, the outer gradient and
the NLL over the positions inside a query song: train / train_indexed / eval read Episode.support_len / query_len or the lengths
handed to attach_table, generate / beam_search / score take support_len=, and a missing length is a ValueError),
maml_per_artist (default false: every path is what it was; true: the episode is a meta-batch of N tasks, DESIGN.md 27 -- train /
train_indexed / eval / eval_many adapt once per artist, on that artist's support songs alone, and report the mean over the artists of
the query NLL at that artist's theta', which is the procedure generate / beam_search / score run for one artist; works with
maml_lengths).
"""
import numpy as np

from models.lstm_baseline import LSTMBaseline


class MAMLLSTM(LSTMBaseline):
    MASKS_PADDING = False        # `mask_padding: true` (the baseline's one-pass loss) is refused at construction; cfg-E's key is maml_lengths
    maml_per_artist = False      # config key `maml_per_artist`: one adaptation per artist in train / train_indexed / eval
    def __init__(self, config):
        super(MAMLLSTM, self).__init__(config)
        self.maml_lengths = bool(config.get('maml_lengths', False))
        self.maml_per_artist = bool(config.get('maml_per_artist', False))
        self._inner_steps = int(config.get('inner_steps', 1))
        self._inner_lr = float(config.get('inner_lr', 0.1))
        if self._inner_steps < 0 or self._inner_lr < 0:
            raise RuntimeError('inner_steps and inner_lr must be >= 0')

    def _episode_lengths(self, episode, which):
        """the episode's lengths as int32 [N, K] / [N, Q], checked against its tokens (maml_lengths)"""
        for name in which:
            if getattr(episode, name + '_len', None) is None:
                raise ValueError('maml_lengths is on and the episode has no %s_len: lengths come from EpisodeSampler.gather '
                                 '(or Episode(support, query, support_len, query_len))' % name)
        return self._lengths(episode, which)

    def _support_lengths(self, support, support_len):
        """support_len of generate / beam_search / score as int32 [rows] (maml_lengths: required; off: refused)"""
        if not self.maml_lengths:
            if support_len is not None:
                raise ValueError('support_len needs maml_lengths: true in the model config')
            return {}
        if support_len is None:
            raise ValueError('maml_lengths is on: the support set needs its lengths (support_len=)')
        ln = np.ascontiguousarray(support_len, dtype=np.int32).reshape(-1)
        if ln.size != support.shape[0]:
            raise ValueError('support_len %r does not match the %d support songs' % (np.shape(support_len), support.shape[0]))
        return dict(support_len=ln)

    def attach_table(self, split, table, lengths=None):
        """like LSTMBaseline.attach_table; with maml_lengths the table's lengths (Dataset.length_table) are needed and uploaded"""
        if self.maml_lengths and lengths is None:
            raise ValueError('maml_lengths is on: attach_table needs the lengths of the table (Dataset.length_table)')
        self._model.upload_table(self.TABLE_IDS[split], table, lengths if self.maml_lengths else None)

    def train(self, episode):
        self._require_init()
        kw = dict(maml_lengths=tuple(self._episode_lengths(episode, ('support', 'query')))) if self.maml_lengths else {}
        if self.maml_per_artist:
            kw['maml_tasks'] = True
        loss = self._parallel.train_step(self._tokens(episode.support, 3), self._tokens(episode.query, 3),
                                         maml=(self._inner_steps, self._inner_lr), **kw)
        self._log_scalar('Train/loss', loss, self._train_calls)
        self._train_calls += 1
        return loss

    # train.train's fast path (episodes as row indices into the split's device-resident token table, losses left on the device): the
    # inherited LSTMBaseline.train_indexed would run the PLAIN baseline step -- inner loop skipped, training and evaluation
    # silently disagreeing.  The table lives on the device like the baseline's (inherited attach_table): the episode's
    # rows are gathered there once and both passes of the step read them in place (fsmg_maml_step_indexed).
    def train_indexed(self, split, support_idx, query_idx, want_loss=False):
        import numpy as np
        self._require_init()
        loss = self._parallel.train_step(np.ascontiguousarray(support_idx, dtype=np.int32),
                                         np.ascontiguousarray(query_idx, dtype=np.int32), want_loss=want_loss,
                                         table=self.TABLE_IDS[split], maml=(self._inner_steps, self._inner_lr),
                                         **(dict(maml_lengths=True) if self.maml_lengths else {}),
                                         **(dict(maml_tasks=True) if self.maml_per_artist else {}))
        if want_loss:
            self._log_scalar('Train/loss', loss, self._train_calls)
        self._train_calls += 1
        return loss

    def eval(self, episode):
        self._require_init()
        if self.maml_per_artist:
            sl, ql = self._episode_lengths(episode, ('support', 'query')) if self.maml_lengths else (None, None)
            nll = self._model.maml_tasks_eval(self._tokens(episode.support, 3), self._tokens(episode.query, 3),
                                              self._inner_steps, self._inner_lr, support_len=sl, query_len=ql)
        elif self.maml_lengths:
            sl, ql = self._episode_lengths(episode, ('support', 'query'))
            nll = self._model.maml_eval_masked(self._tokens(episode.support, 3), self._tokens(episode.query, 3), sl, ql,
                                               self._inner_steps, self._inner_lr)
        else:
            nll = self._model.maml_eval(self._tokens(episode.support, 3), self._tokens(episode.query, 3),
                                        self._inner_steps, self._inner_lr)
        self._log_scalar('Eval/Avg_NLL', nll, self._eval_calls)
        self._eval_calls += 1
        return nll

    def generate(self, support_set, num, n=1, temperature=1.0, top_k=0, seed=0, primer_len=0, logprobs=False, top_p=0.0, min_p=0.0, repetition_penalty=1.0, repeat_window=0,
                 support_len=None, constraints=None, cstate=None, return_cstate=False):
        """like LSTMBaseline.generate, at theta' = theta adapted on the support set (inner_steps, inner_lr); theta is restored.
        support_len [rows]: the support songs' lengths (maml_lengths).  constraints, cstate, return_cstate: LSTMBaseline.generate's
        (include/fsmg.h fsmg_maml_generate_constrained)"""
        self._require_init()
        support = self._tokens(support_set, 2)
        con = dict(constraints=constraints, cstate=cstate, return_cstate=return_cstate) if constraints is not None else {}
        if constraints is None and (cstate is not None or return_cstate):
            raise ValueError('cstate / return_cstate need constraints')
        return self._model.maml_generate(support, int(num), self._inner_steps, self._inner_lr, n_seq=int(n),
                                         temperature=temperature, top_k=top_k, seed=seed,
                                         primer=self._primer(support, int(n), int(primer_len)), logprobs=logprobs,
                                         top_p=top_p, min_p=min_p, repetition_penalty=repetition_penalty, repeat_window=repeat_window,
                                         **self._support_lengths(support, support_len), **con)

    def beam_search(self, support_set, num, beam_width, n=1, primer_len=0, logprobs=False, support_len=None, constraints=None,
                    cstate=None, return_cstate=False):
        """like LSTMBaseline.beam_search, at theta' = theta adapted on the support set (inner_steps, inner_lr); theta is restored.
        support_len [rows]: the support songs' lengths (maml_lengths).  constraints, cstate, return_cstate: LSTMBaseline.beam_search's
        (fsmg_maml_beam_search_constrained)"""
        self._require_init()
        support = self._tokens(support_set, 2)
        if constraints is None and (cstate is not None or return_cstate):
            raise ValueError('cstate / return_cstate need constraints')
        con = dict(constraints=constraints, cstate=cstate, return_cstate=return_cstate) if constraints is not None else {}
        return self._model.maml_beam_search(support, int(num), self._inner_steps, self._inner_lr, int(beam_width), n_groups=int(n),
                                            primer=self._primer(support, int(n), int(primer_len)), logprobs=logprobs,
                                            **self._support_lengths(support, support_len), **con)

    def score(self, support_set, songs, support_len=None, **kw):
        """like LSTMBaseline.score, at theta' = theta adapted on the support set (inner_steps, inner_lr); theta is restored.
        support_len [rows]: the support songs' lengths (maml_lengths); lengths= then gives the scored songs' own"""
        self._require_init()
        support = self._tokens(support_set, 2)
        return self._model.maml_score(support, songs, self._inner_steps, self._inner_lr, **self._support_lengths(support, support_len), **kw)

    def eval_many(self, episodes):
        """adaptation is per episode, so there is nothing to batch: one maml_eval per episode"""
        return [self.eval(e) for e in episodes]
