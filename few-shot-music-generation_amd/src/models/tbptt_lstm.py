"""LSTM baseline trained and evaluated over SEGMENTS of its songs: truncated BPTT on a carried state (include/fsmg.h
fsmg_*_state).

The data's songs have `max_len` tokens; the handle is created with max_len = `segment_len`, so a song may be many times longer than
one pass of the library.  An episode's songs are walked in ceil(max_len / segment_len) segments on ONE decode state (one row per
song, reset per episode): every segment starts from the hidden state the previous one ended in and reads the previous segment's last
token first.

  train(episode)  one clip + Adam update per segment (fsmg_train_step_state): the gradient of a segment holds the incoming state
                  constant -- truncated BPTT.  Returns the episode's mean NLL over all scored positions, each segment under the
                  weights it was computed with.
  eval(episode)   the query songs' NLL under FULL context, exact: the segments' NLL numerators summed over the total n_valid
                  (fsmg_eval_step_state) -- the number a handle with max_len = the songs' length would report, to rounding.

Model key `segment_len` (required).  With `mask_padding: true` the songs' lengths (Episode.support_len / query_len, the .len.npy
sidecars) bound the scored positions; the last segment of a song is ragged through the pass's lengths, and a segment no song reaches
is not run.  Without it every position of every song is scored, as in LSTMBaseline.  Everything LSTMBaseline offers that reads songs
of the HANDLE's max_len (sample, generate, score, ...) is inherited at segment_len.  The index fast path of train.train (a
device-resident table of whole songs) and episode-parallel training are not offered: train.train takes the episode path.
"""
import numpy as np

from models.lstm_baseline import LSTMBaseline


def segment_plan(song_len, lengths, segment_len):
    """-> [(first token, per-row lengths int32 [R])] of the segments that score anything: lengths [R] in [0, song_len]"""
    lengths = np.asarray(lengths, np.int64)
    plan = []
    for s0 in range(0, int(song_len), int(segment_len)):
        ln = np.clip(lengths - s0, 0, segment_len).astype(np.int32)
        if ln.sum() == 0:
            break
        plan.append((s0, ln))
    return plan


def segment_tokens(songs, s0, segment_len):
    """songs int32 [R, song_len] -> the segment's [R, segment_len] block, zeros behind the songs' end"""
    out = np.zeros((songs.shape[0], segment_len), np.int32)
    part = songs[:, s0:s0 + segment_len]
    out[:, :part.shape[1]] = part
    return out


class TBPTTLSTM(LSTMBaseline):
    def __init__(self, config):
        if 'segment_len' not in config:
            raise RuntimeError('required config key "segment_len" not found')
        self._song_len = int(config['max_len'])
        self._segment_len = int(config['segment_len'])
        if not (1 <= self._segment_len <= self._song_len):
            raise RuntimeError('segment_len must be in [1, max_len], got %d with max_len %d' % (self._segment_len, self._song_len))
        handle_config = dict(config)
        handle_config['max_len'] = self._segment_len       # what one pass of the library reads
        super(TBPTTLSTM, self).__init__(handle_config)
        if self._parallel.world > 1:
            raise RuntimeError('TBPTTLSTM trains in one process (a state pass refuses the library-owned exchange, include/fsmg.h)')
        self._states = {}

    # train.train asks for these by name: without them it takes the episode path (train / eval below)
    @property
    def attach_table(self):
        raise AttributeError('TBPTTLSTM has no index fast path: its songs are longer than the handle\'s max_len')

    @property
    def train_indexed(self):
        raise AttributeError('TBPTTLSTM has no index fast path: its songs are longer than the handle\'s max_len')

    @property
    def n_segments(self):
        return -(-self._song_len // self._segment_len)

    def _state(self, rows):
        """the decode state of `rows` rows, fresh"""
        st = self._states.get(rows)
        if st is None:
            st = self._states[rows] = self._model.new_state(rows, history=1)
        st.reset()
        return st

    def _songs(self, episode, names):
        """-> songs int32 [R, song_len], lengths int64 [R] of the named sets, support rows first"""
        songs, lens = [], []
        for name in names:
            tok = self._tokens(getattr(episode, name), 3)
            if tok.shape[2] != self._song_len:
                raise ValueError('%s %r does not match max_len=%d' % (name, tok.shape, self._song_len))
            songs.append(tok.reshape(-1, self._song_len))
            if self.mask_padding:
                # (the base class checks lengths against ITS max_len, the segment's: here a song's length may reach the song's)
                ln = getattr(episode, name + '_len', None)
                if ln is None:
                    raise ValueError('mask_padding is on and the episode has no %s_len' % name)
                ln = np.asarray(ln, np.int64).reshape(-1)
                if ln.size != songs[-1].shape[0] or ln.min() < 1 or ln.max() > self._song_len:
                    raise ValueError('%s_len must hold one length in [1, %d] per song' % (name, self._song_len))
                lens.append(ln)
            else:
                lens.append(np.full(songs[-1].shape[0], self._song_len, np.int64))
        return np.concatenate(songs), np.concatenate(lens)

    def _walk(self, songs, lengths, step):
        """step(state, tokens, lengths) -> NLL of the segment over its n_valid; -> the NLL over all scored positions"""
        state = self._state(songs.shape[0])
        total, n = 0.0, 0
        for s0, ln in segment_plan(self._song_len, lengths, self._segment_len):
            nv = int(ln.sum())
            total += float(step(state, segment_tokens(songs, s0, self._segment_len), ln)) * nv
            n += nv
        return total / n

    def train(self, episode):
        self._require_init()
        songs, lengths = self._songs(episode, ('support', 'query'))
        loss = self._walk(songs, lengths, self._model.train_step_state)
        self._log_scalar('Train/loss', loss, self._train_calls)
        self._train_calls += 1
        return loss

    def eval(self, episode):
        self._require_init()
        songs, lengths = self._songs(episode, ('query',))
        nll = self._walk(songs, lengths, lambda st, tok, ln: self._model.eval_step_state(st, tok, ln)[0])
        self._log_scalar('Eval/Avg_NLL', nll, self._eval_calls)
        self._eval_calls += 1
        return nll

    def eval_many(self, episodes):
        return [self.eval(e) for e in episodes]
