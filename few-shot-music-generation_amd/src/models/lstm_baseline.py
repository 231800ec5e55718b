"""LSTM language-model baseline -- MI355X-native plugin.

Drop-in for /root/reference/src/models/lstm_baseline.py: same module path and class name
(`model_module_name: models.lstm_baseline`, `model_class_name: LSTMBaseline`), same config
keys, same six plugin members with the same meaning -- but the TensorFlow graph and session
are replaced by libfsmg (hand-written gfx950 kernels behind include/fsmg.h):

  train(episode)  support + query flattened support-first, one clip+Adam update, returns the
                  mean NLL under the PRE-update weights      (reference :89-113)
  eval(episode)   query-only mean NLL, no state change       (reference :115-133)
  sample(s, num)  greedy argmax decode from the start word; the support set is ignored, as in
                  the reference                              (reference :135-156)

Beyond the reference: generate(s, num, n, temperature, top_k, seed, primer_len) draws n samples at once on the device,
optionally continuing the first primer_len tokens of the support songs; beam_search(s, num, beam_width, n, primer_len) returns
the beam_width highest-scoring continuations of each of n groups, searched on the device; score(s, songs, ...) reads given songs
and returns per-token log-probabilities, ranks of the true token, predictive entropies, argmaxes and per-song NLLs (the support set
is ignored, as in sample).  condition(s) reads the support songs into a decode state, one row per artist (include/fsmg.h
fsmg_dstate_*); generate(..., condition_on_support=True) continues from it, and eval_conditioned(episode) is the few-shot baseline
that reads the support set before it scores the query songs.

Optional config keys beyond the reference's: device, clip_norm_mode ('tf1_slices' | 'dense'),
max_sequences, use_graph, gemm / schedule / recurrence / dp_split_backward (fsmg_config), dp_exchange ('torch': the
all-reduce is issued through torch.distributed; 'library': libfsmg issues the RCCL calls itself), mask_padding (default false; true:
train / train_indexed / eval / eval_many score position t of a song iff t < its length -- Episode.support_len / query_len, the
lengths handed to attach_table -- and average over the scored positions, include/fsmg.h "per-song lengths"),
keep_prob_input / keep_prob_output / dropout_variational / dropout_seed (config/lstm_dropout.yaml; all absent by default = never
enabled: dropout of the train passes on the non-recurrent connections, include/fsmg.h "Dropout"; eval, sample, generate, score never
drop; rank r of an episode-parallel run draws its masks from fsmg.dist.rank_seed(dropout_seed, r); the index of the next dropped pass
is saved and restored next to the native checkpoint, <name>.dropout.npz -- ONE file holding the index at the latest save, while the
native checkpoints are kept per step: recovering from an older checkpoint than the newest restores the newest index, i.e. the run
continues with masks of later passes, not the ones it drew the first time; every rank of an episode-parallel run writes the same
file with the same counter, atomically).  When torch.distributed is initialised, train() runs
episode-parallel (one episode per rank, one gradient all-reduce per step, see fsmg/dist.py).
"""
import os

import numpy as np

from fsmg.dist import EpisodeParallel, rank_seed
from models.hip_model import HIPModel

DROPOUT_KEYS = ('keep_prob_input', 'keep_prob_output', 'dropout_variational', 'dropout_seed')


def dropout_settings(config, rank=0):
    """the dropout keys of a model config -> the keyword arguments of FsmgModel.dropout_enable for rank `rank`, or None when none of the
    keys is there (the handle is then never enabled)"""
    if not any(config.get(k) is not None for k in DROPOUT_KEYS):
        return None
    keep_in = float(config['keep_prob_input']) if config.get('keep_prob_input') is not None else 1.0
    keep_out = float(config['keep_prob_output']) if config.get('keep_prob_output') is not None else 1.0
    for name, k in (('keep_prob_input', keep_in), ('keep_prob_output', keep_out)):
        if not (0.0 < k <= 1.0):
            raise RuntimeError('%s must be in (0, 1], got %r' % (name, k))
    seed = int(config.get('dropout_seed') or 0)
    if seed < 0:
        raise RuntimeError('dropout_seed must be >= 0')
    return dict(keep_input=keep_in, keep_output=keep_out, variational=bool(config.get('dropout_variational') or False),
                seed=rank_seed(seed, rank))


def save_dropout(engine, path):
    """the index the engine's next dropped pass takes -> one small .npz beside the native checkpoint (which stays byte-identical)"""
    tmp = path + '.tmp.npz'
    np.savez(tmp, next_pass=np.int64(engine.dropout_info()['next_pass']))
    os.replace(tmp, path)


def load_dropout(engine, path):
    """-> True when the file exists and holds an index (the engine's next dropped pass then takes it), else False with nothing set"""
    if not os.path.isfile(path):
        return False
    with np.load(path) as blob:
        if 'next_pass' not in blob or int(blob['next_pass']) < 0:
            return False
        engine.dropout_set_pass(int(blob['next_pass']))
    return True


class LSTMBaseline(HIPModel):
    MASKS_PADDING = True         # a subclass that has no masked form says so: it refuses `mask_padding: true` instead of ignoring it

    def __init__(self, config):
        self.mask_padding = bool(config.get('mask_padding', False))
        if self.mask_padding and not self.MASKS_PADDING:
            raise RuntimeError('%s has no padding-masked loss: mask_padding: true is supported by LSTMBaseline only '
                               '(remove the key or set it to false)' % type(self).__name__)
        for key in ('name', 'input_size', 'max_len', 'embedding_size', 'hidden_size', 'n_layers',
                    'lr', 'max_grad_norm', 'n_decay'):
            if key not in config:
                raise RuntimeError('required config key "%s" not found' % key)
        super(LSTMBaseline, self).__init__(config)
        self._start_word = int(config['input_size'])
        self._time_steps = int(config['max_len'])
        self._parallel = EpisodeParallel(self)
        if config.get('dp_exchange', 'torch') == 'library' and self._parallel.world > 1:
            self.attach_library_comm()
        self._dropout = dropout_settings(config, self._parallel.rank)

    def _dropout_path(self, checkpt_path):
        return os.path.join(checkpt_path, self.name, self.name + '.dropout.npz')

    def save(self, checkpt_path):
        super(LSTMBaseline, self).save(checkpt_path)
        if self._dropout is not None:
            save_dropout(self._model, self._dropout_path(checkpt_path))

    def recover_or_init(self, init_path):
        super(LSTMBaseline, self).recover_or_init(init_path)
        if self._parallel.world > 1:                     # replicas start from rank 0's state
            self._parallel.broadcast_parameters(self._arena)
        if self._dropout is not None:                    # the gradient passes of the train forms are dropped from here on
            self._model.dropout_enable(**self._dropout)
            if init_path and load_dropout(self._model, self._dropout_path(init_path)):
                print('recovered the dropout pass index')

    @staticmethod
    def _tokens(arr, ndim):
        a = np.ascontiguousarray(arr, dtype=np.int32)
        if a.ndim != ndim:
            raise ValueError('expected a %d-d token array, got shape %r' % (ndim, a.shape))
        return a

    def _lengths(self, episode, which):
        """the episode's lengths as int32 [N, K] / [N, Q], checked against its tokens (mask_padding)"""
        out = []
        for name in which:
            ln, tokens = getattr(episode, name + '_len', None), getattr(episode, name)
            if ln is None:
                raise ValueError('mask_padding is on and the episode has no %s_len: lengths come from EpisodeSampler.gather '
                                 '(or Episode(support, query, support_len, query_len))' % name)
            ln = np.ascontiguousarray(ln, dtype=np.int32)
            if ln.shape != tuple(np.shape(tokens)[:2]):
                raise ValueError('%s_len %r does not match the length of %s %r' % (name, ln.shape, name, np.shape(tokens)))
            out.append(ln)
        return out

    def train(self, episode):
        self._require_init()
        kw = dict(lengths=tuple(self._lengths(episode, ('support', 'query')))) if self.mask_padding else {}
        loss = self._parallel.train_step(self._tokens(episode.support, 3), self._tokens(episode.query, 3), **kw)
        self._log_scalar('Train/loss', loss, self._train_calls)
        self._train_calls += 1
        return loss

    # -- fast path of train.train: episodes as row indices into a device-resident split table, losses left on the device --
    TABLE_IDS = {'train': 0, 'val': 1, 'test': 2}

    def attach_table(self, split, table, lengths=None):
        """Upload the packed [n_songs, max_len] int32 token table of a split (data.dataset.Dataset.token_table) once; episodes
        of that split can then be given as row indices (train_indexed).  lengths: int32 [n_songs]
        (data.dataset.Dataset.length_table), needed when mask_padding is on."""
        if self.mask_padding and lengths is None:
            raise ValueError('mask_padding is on: attach_table needs the lengths of the table (Dataset.length_table)')
        self._model.upload_table(self.TABLE_IDS[split], table, lengths if self.mask_padding else None)

    def train_indexed(self, split, support_idx, query_idx, want_loss=False):
        """Same step as train(episode) for the episode table[support_idx], table[query_idx]; with want_loss=False nothing is
        read back (the loss goes to the device ring: recent_losses) and the host does not wait for the GPU."""
        self._require_init()
        loss = self._parallel.train_step(np.ascontiguousarray(support_idx, dtype=np.int32),
                                         np.ascontiguousarray(query_idx, dtype=np.int32), want_loss=want_loss,
                                         table=self.TABLE_IDS[split], **(dict(lengths=True) if self.mask_padding else {}))
        if want_loss:
            self._log_scalar('Train/loss', loss, self._train_calls)
        self._train_calls += 1
        return loss

    def recent_losses(self, n):
        """the last n (<= 1024) train losses, oldest first; synchronises"""
        return self._model.read_losses(int(n))

    def global_step(self):
        """train steps the device has really applied (a skipped step does not count); synchronises"""
        return self._model.step

    def log_deferred_losses(self, losses):
        """Train/loss scalars of steps that ran with want_loss=False, written when train.train folds them in"""
        # labelled by the step the device really applied (global_step counts those; a skipped step leaves no loss behind), so the
        # window's last loss carries the current global_step - 1
        first = self._model.step - len(losses)
        for i, loss in enumerate(losses):
            self._log_scalar('Train/loss', float(loss), max(first + i, 0))

    def eval(self, episode):
        self._require_init()
        if self.mask_padding:
            nll = self._model.eval_step_masked(self._tokens(episode.query, 3), self._lengths(episode, ('query',))[0])
        else:
            nll = self._model.eval_step(self._tokens(episode.query, 3))
        self._log_scalar('Eval/Avg_NLL', nll, self._eval_calls)
        self._eval_calls += 1
        return nll

    def eval_many(self, episodes):
        """[model.eval(e) for e in episodes] in one device pass (episodes must share N, Q)."""
        self._require_init()
        queries = np.stack([self._tokens(e.query, 3) for e in episodes])
        if self.mask_padding:
            nlls = self._model.eval_batch_masked(queries, np.stack([self._lengths(e, ('query',))[0] for e in episodes]))
        else:
            nlls = self._model.eval_batch(queries)
        for nll in nlls:
            self._log_scalar('Eval/Avg_NLL', float(nll), self._eval_calls)
            self._eval_calls += 1
        return [float(x) for x in nlls]

    def sample(self, support_set, num):
        self._require_init()
        return self._model.sample(int(num))

    @staticmethod
    def _primer(support_set, n, primer_len):
        """the first primer_len tokens of the support songs, dealt round-robin over the n rows"""
        if primer_len <= 0:
            return None
        songs = np.ascontiguousarray(support_set, dtype=np.int32).reshape(-1, np.shape(support_set)[-1])
        if primer_len > songs.shape[1]:
            raise ValueError('primer_len %d exceeds the song length %d' % (primer_len, songs.shape[1]))
        return np.ascontiguousarray(songs[np.arange(n) % songs.shape[0], :primer_len])

    def condition(self, support_set, history=None):
        """Read the support songs into a decode state (fsmg.binding.DecodeState): support_set int32 [A, K, max_len] (or
        [K, max_len]: one artist) -> a state of A rows, row a having read song_1, then [start] + song_k for k = 2..K of artist a.
        Every song has max_len tokens, so the rows stay in lockstep.  history: context tokens the state keeps (the repetition
        penalty's reach); default: everything condition reads plus 2 * max_len.  The caller closes the state."""
        self._require_init()
        s = np.ascontiguousarray(support_set, dtype=np.int32)
        if s.ndim == 2:
            s = s[None]
        if s.ndim != 3 or s.shape[2] != self._time_steps:
            raise ValueError('support_set must be [A, K, %d] or [K, %d], got %r' % (self._time_steps, self._time_steps, s.shape))
        A, K, T = s.shape
        state = self._model.new_state(A, history=int(history) if history else K * (T + 1) + 2 * T)
        start = np.full((A, 1), self._start_word, np.int32)
        for k in range(K):
            self._model.feed(state, s[:, k] if k == 0 else np.concatenate([start, s[:, k]], axis=1))
        return state

    def eval_conditioned(self, episode):
        """The few-shot baseline that reads the support set: artist a's support songs are read into a decode state (condition), the
        state is copied to the artist's Q query rows, and each row is fed [start] + its query song with log-probs.  -> the mean NLL
        of the N * Q * max_len query-song tokens (the start word's own log-prob is dropped): eval's number, with every query song
        scored behind its artist's support songs instead of from a zero state.  No backward pass, no state change of the model."""
        self._require_init()
        query = self._tokens(episode.query, 3)
        N, Q, T = query.shape
        support = self._tokens(episode.support, 3)
        if support.shape[0] != N or T != self._time_steps:
            raise ValueError('support %r / query %r do not match max_len=%d' % (support.shape, query.shape, self._time_steps))
        state = self.condition(support)
        rows = self._model.new_state(N * Q, history=state.history)
        try:
            rows.gather(state, np.repeat(np.arange(N), Q))
            start = np.full((N * Q, 1), self._start_word, np.int32)
            lp = self._model.feed(rows, np.concatenate([start, query.reshape(N * Q, T)], axis=1), logprobs=True)
        finally:
            rows.close()
            state.close()
        return float(-np.mean(lp[:, 1:].astype(np.float64)))

    def generate(self, support_set, num, n=1, temperature=1.0, top_k=0, seed=0, primer_len=0, logprobs=False, top_p=0.0, min_p=0.0, repetition_penalty=1.0, repeat_window=0,
                 condition_on_support=False, _draw=None, constraints=None, cstate=None, return_cstate=False):
        """n independent samples of num tokens (int32 [n, num]), drawn on the device (temperature, top_k, seed; include/fsmg.h
        fsmg_generate).  Each row continues the first primer_len tokens of a support song (dealt round-robin); with
        primer_len 0 the support set is not used.  top_p, min_p, repetition_penalty, repeat_window: the sampling filters
        (include/fsmg.h fsmg_generate_filtered; all off by default).
        condition_on_support=True: the support songs are read first (condition: one state row per artist, dealt round-robin over the
        n rows), then [start] and the first primer_len tokens of one of that artist's support songs, and the rows continue from
        there.  (_draw: what stands in for FsmgModel.generate -- a subclass's own decoder with the same keywords.)
        constraints: a data.constraints.Constraints (e.g. MIDILoader.constraints()) restricting what may be drawn (include/fsmg.h
        fsmg_generate_constrained); the primer must be allowed by it.  cstate / return_cstate: FsmgModel.generate's."""
        self._require_init()
        draw = _draw if _draw is not None else self._model.generate
        if constraints is not None:       # (only then: a stand-in decoder need not know these keywords)
            if _draw is not None:
                raise ValueError('constraints are not supported by this decoder')
            base = draw
            draw = lambda *a, **kw: base(*a, constraints=constraints, cstate=cstate, return_cstate=return_cstate, **kw)
        elif cstate is not None or return_cstate:
            raise ValueError('cstate / return_cstate need constraints')
        if condition_on_support:
            n, num = int(n), int(num)
            K, T = np.shape(support_set)[-2:]
            # room for everything the rows will have read, so that a whole-context penalty (repeat_window 0) reaches all of it
            state = self.condition(support_set, history=K * (T + 1) + 1 + int(primer_len) + num)
            rows = self._model.new_state(n, history=state.history)
            try:
                rows.gather(state, np.arange(n) % state.rows)
                # row i continues artist i % A: [start], then the first primer_len tokens of one of that artist's own songs
                songs = np.ascontiguousarray(support_set, dtype=np.int32).reshape(state.rows, K, T)
                i = np.arange(n)
                if int(primer_len) > T:
                    raise ValueError('primer_len %d exceeds the song length %d' % (primer_len, T))
                head = np.full((n, 1), self._start_word, np.int32)
                self._model.feed(rows, np.concatenate([head, songs[i % state.rows, (i // state.rows) % K, :max(int(primer_len), 0)]], axis=1))
                return draw(n, num, temperature=temperature, top_k=top_k, seed=seed, logprobs=logprobs, top_p=top_p,
                            min_p=min_p, repetition_penalty=repetition_penalty, repeat_window=repeat_window, state=rows)
            finally:
                rows.close()
                state.close()
        return draw(int(n), int(num), temperature=temperature, top_k=top_k, seed=seed,
                    primer=self._primer(support_set, int(n), int(primer_len)), logprobs=logprobs,
                    top_p=top_p, min_p=min_p, repetition_penalty=repetition_penalty, repeat_window=repeat_window)

    def beam_search(self, support_set, num, beam_width, n=1, primer_len=0, logprobs=False, constraints=None, cstate=None,
                    return_cstate=False):
        """n independent beam searches of width beam_width, num tokens each, on the device (include/fsmg.h fsmg_beam_search):
        -> tokens int32 [n, beam_width, num], scores float32 [n, beam_width] (, per-token log-probs with logprobs=True), best
        first.  Group i continues the first primer_len tokens of a support song, dealt round-robin like generate's rows.
        constraints: a data.constraints.Constraints the search ranks under (fsmg_beam_search_constrained); cstate / return_cstate:
        the groups' constraint states to start from and the hypotheses' final ones, as in FsmgModel.beam_search."""
        self._require_init()
        if constraints is None and (cstate is not None or return_cstate):
            raise ValueError('cstate / return_cstate need constraints')
        con = dict(constraints=constraints, cstate=cstate, return_cstate=return_cstate) if constraints is not None else {}
        return self._model.beam_search(int(num), int(beam_width), n_groups=int(n),
                                       primer=self._primer(support_set, int(n), int(primer_len)), logprobs=logprobs, **con)

    def score(self, support_set, songs, **kw):
        """Per-token statistics of the given songs (int32 [R, max_len]) under the model (include/fsmg.h fsmg_score): a dict of
        'logprob' / 'row_nll' and, on request (rank=True, entropy=True, argmax=True), 'rank', 'entropy', 'argmax'.  The support
        set is ignored, as in sample.  Keywords: FsmgModel.score's."""
        self._require_init()
        return self._model.score(songs, **kw)
