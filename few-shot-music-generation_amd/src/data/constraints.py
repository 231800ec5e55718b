"""Decoding constraints (include/fsmg.h "constrained decoding"): the host-side tables of one fsmg_constraint and
their semantics in plain numpy, usable without a GPU.

A constraint restricts the columns a pick may draw through three independent mechanisms:
    bias        float [V1] added to the logit, -inf bans a column
    automaton   token_class [V1] in [0, C), next_state [S, C] in [-1, S) (-1 forbids the class in that state), start_state
    slots       slot_open / slot_close [V1] in [-1, K): a token that opens slot k is allowed only while k is closed, one that closes
                it only while it is open
A row's state is (state, open) with open a uint32 [ceil(K / 32)] bitset, bit k = bit k & 31 of word k >> 5.
"""
import numpy as np

MAX_STATES, MAX_CLASSES, MAX_SLOTS = 256, 64, 4096


class Constraints(object):
    def __init__(self, n_columns, bias=None, token_class=None, next_state=None, start_state=0, slot_open=None, slot_close=None,
                 n_slots=0):
        V1 = self.n_columns = int(n_columns)
        self.bias = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32).reshape(V1)
        if (token_class is None) != (next_state is None):
            raise ValueError('token_class and next_state come together')
        self.token_class = None if token_class is None else np.ascontiguousarray(token_class, dtype=np.int32).reshape(V1)
        self.next_state = None if next_state is None else np.ascontiguousarray(next_state, dtype=np.int32)
        self.start_state = int(start_state)
        self.n_slots = int(n_slots)
        self.slot_open = None if slot_open is None else np.ascontiguousarray(slot_open, dtype=np.int32).reshape(V1)
        self.slot_close = None if slot_close is None else np.ascontiguousarray(slot_close, dtype=np.int32).reshape(V1)
        self.validate()

    # ---- shape
    @property
    def n_states(self):
        return 1 if self.next_state is None else self.next_state.shape[0]

    @property
    def n_classes(self):
        return 1 if self.next_state is None else self.next_state.shape[1]

    @property
    def n_words(self):
        return (self.n_slots + 31) // 32

    def validate(self):
        """what fsmg_constraint_create refuses, as a ValueError"""
        S, C, K = self.n_states, self.n_classes, self.n_slots
        if self.next_state is not None and self.next_state.ndim != 2:
            raise ValueError('next_state must be [S, C]')
        if not (1 <= S <= MAX_STATES and 1 <= C <= MAX_CLASSES and 0 <= K <= MAX_SLOTS):
            raise ValueError('limits: 1 <= S <= 256, 1 <= C <= 64, 0 <= K <= 4096')
        if not 0 <= self.start_state < S:
            raise ValueError('start_state outside [0, S)')
        if self.bias is not None and (np.isnan(self.bias).any() or (self.bias == np.inf).any()):
            raise ValueError('bias must be finite or -inf')
        if self.token_class is not None:
            if self.token_class.min() < 0 or self.token_class.max() >= C:
                raise ValueError('token_class outside [0, C)')
            if self.next_state.min() < -1 or self.next_state.max() >= S:
                raise ValueError('next_state outside [-1, S)')
        for a in (self.slot_open, self.slot_close):
            if a is not None and (a.min() < -1 or a.max() >= K):
                raise ValueError('slot index outside [-1, K)')
        if self.slot_open is not None and self.slot_close is not None and ((self.slot_open >= 0) & (self.slot_close >= 0)).any():
            raise ValueError('a token both opens and closes a slot')

    # ---- state
    def initial(self):
        """-> (start state, every slot closed)"""
        return self.start_state, np.zeros(self.n_words, np.uint32)

    def _bits(self, open_words, slots):
        """the open bit of each slot index in `slots` (entries < 0: False)"""
        k = np.maximum(slots, 0)
        words = np.asarray(open_words, np.uint32)
        if words.size == 0:
            return np.zeros(slots.shape, bool)
        return ((words[k >> 5] >> (k & 31).astype(np.uint32)) & np.uint32(1)).astype(bool) & (slots >= 0)

    def allowed(self, state, open_words):
        """bool [V1]: the allowed set Omega in (state, open)"""
        ok = np.ones(self.n_columns, bool)
        if self.bias is not None:
            ok &= self.bias > -np.inf
        if self.token_class is not None:
            ok &= self.next_state[int(state)][self.token_class] >= 0
        if self.slot_open is not None:
            ok &= ~((self.slot_open >= 0) & self._bits(open_words, self.slot_open))
        if self.slot_close is not None:
            ok &= ~((self.slot_close >= 0) & ~self._bits(open_words, self.slot_close))
        return ok

    def token_allowed(self, state, open_words, token):
        v = int(token)
        if not 0 <= v < self.n_columns:
            return False
        if self.bias is not None and not self.bias[v] > -np.inf:
            return False
        if self.token_class is not None and self.next_state[int(state), self.token_class[v]] < 0:
            return False
        for a, want_open in ((self.slot_open, False), (self.slot_close, True)):
            if a is not None and a[v] >= 0:
                k = int(a[v])
                if bool((int(open_words[k >> 5]) >> (k & 31)) & 1) != want_open:
                    return False
        return True

    def advance(self, state, open_words, token):
        """the state after drawing `token` (which must be allowed) -> (state, open); the input bitset is not modified"""
        v = int(token)
        s = int(state) if self.token_class is None else int(self.next_state[int(state), self.token_class[v]])
        o = np.array(open_words, np.uint32)
        for a in (self.slot_open, self.slot_close):
            if a is not None and a[v] >= 0:
                k = int(a[v])
                o[k >> 5] ^= np.uint32(1 << (k & 31))
        return s, o

    def first_violation(self, tokens, state=None, open_words=None):
        """index of the first token that is not allowed where it stands (walking from the given or the initial state), or None"""
        s, o = self.initial()
        if state is not None:
            s = int(state)
        if open_words is not None:
            o = np.array(open_words, np.uint32)
        for i, w in enumerate(tokens):
            if not self.token_allowed(s, o, w):
                return i
            s, o = self.advance(s, o, w)
        return None


def midi_constraints(instruments=None, max_silence=None, n_columns=None):
    """The MIDI preset: what the detokenizer keeps (data.midi_loader.detokenize_tokens), not a grammar of the tokenizer's output.
    K = 2048 slots: note-on f * 128 + p opens slot f * 128 + p, its note-off closes it, so every note-off ends a sounding note and no
    note-on overwrites one.  The start word and every column at or above the vocabulary (4708) are banned through the bias.
    instruments: a set of families (0 .. 15, the detokenizer's instrument classes); the other families' note-on and velocity ids are
    banned.  max_silence = n: at most n time-shift tokens in a row (an automaton with states 0 .. n).  No velocity rule: the
    reference tokenizer's velocity bin 32 spills into the next family's bin 0, and the detokenizer accepts any order."""
    from data import midi_loader as M
    V = M.OFF_TIME + M.MAX_SHIFT_STEPS
    V1 = V + 1 if n_columns is None else int(n_columns)
    if V1 < V + 1:
        raise ValueError('the MIDI preset needs at least %d columns' % (V + 1))
    bias = np.zeros(V1, np.float32)
    bias[V:] = -np.inf
    if instruments is not None:
        keep = set(int(f) for f in instruments)
        if not keep <= set(range(M.NUM_FAMILIES)):
            raise ValueError('instruments must be families in [0, %d)' % M.NUM_FAMILIES)
        for f in range(M.NUM_FAMILIES):
            if f not in keep:
                bias[f * M.NUM_PITCHES:(f + 1) * M.NUM_PITCHES] = -np.inf
                bias[M.OFF_VELOCITY + f * M.NUM_VELOCITY_BINS:M.OFF_VELOCITY + (f + 1) * M.NUM_VELOCITY_BINS] = -np.inf
    K = M.OFF_NOTE_OFF
    slot_open = np.full(V1, -1, np.int32)
    slot_close = np.full(V1, -1, np.int32)
    slot_open[:K] = np.arange(K)
    slot_close[K:2 * K] = np.arange(K)
    token_class = next_state = None
    if max_silence is not None:
        n = int(max_silence)
        if not 0 <= n < MAX_STATES:
            raise ValueError('max_silence must be in [0, %d)' % MAX_STATES)
        token_class = np.zeros(V1, np.int32)
        token_class[M.OFF_TIME:V] = 1
        next_state = np.zeros((n + 1, 2), np.int32)             # class 0: back to state 0
        next_state[:, 1] = np.arange(1, n + 2)                  # a time shift: one further
        next_state[n, 1] = -1                                   # ... and none at n
    return Constraints(V1, bias=bias, token_class=token_class, next_state=next_state, slot_open=slot_open, slot_close=slot_close,
                       n_slots=K)
