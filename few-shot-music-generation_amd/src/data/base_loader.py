"""Per-song token loading: the on-disk token format of the reference.

Mirrors the behaviour of the reference `Loader` (/root/reference/src/data/base_loader.py:12-64):
a song file `<path>` has a pre-tokenised sidecar `<path>.<max_len>.npy` (int32
[max_len]); when the sidecar is missing the song is read, tokenised, truncated /
ZERO-padded to max_len (padding is not masked downstream and id 0 is also a real
token -- SURVEY.md Q6) and the sidecar is written.

Beyond the reference: when a song is tokenised, its length goes into a second sidecar `<path>.<max_len>.len.npy` (one int32,
min(max_len, n_tokens), at least 1) for the padding-masked loss (`mask_padding`).  A token sidecar without a length
sidecar -- a tree the reference wrote -- means max_len: nothing is guessed from zeros, because id 0 is a real token.
"""
import os

import numpy as np

_VALIDATION_ERRORS = (OSError, KeyError, EOFError, IndexError, ValueError, IOError)


class Loader(object):
    """Turns a song file into a fixed-length row of token ids."""

    def __init__(self, max_len, dtype=np.int32, persist=True):
        self.max_len = int(max_len)
        self.dtype = dtype
        self.persist = persist

    # -- to be provided by the concrete loader --------------------------------
    def is_song(self, filepath):
        raise NotImplementedError

    def read(self, filepath):
        raise NotImplementedError

    def tokenize(self, data):
        raise NotImplementedError

    def detokenize(self, numpy_data):
        raise NotImplementedError

    def get_num_tokens(self):
        raise NotImplementedError

    def constraints(self, **kw):
        """the decoding constraints of this vocabulary (data.constraints.Constraints), or None when it has none"""
        return None

    # -- shared ------------------------------------------------------------------
    def sidecar_path(self, filepath):
        return '%s.%s.npy' % (filepath, self.max_len)

    def length_sidecar_path(self, filepath):
        return '%s.%s.len.npy' % (filepath, self.max_len)

    def _save_atomically(self, path, array):       # another rank must never np.load a half-written sidecar
        tmp = '%s.%d.tmp.npy' % (path, os.getpid())
        np.save(tmp, array)
        os.replace(tmp, path)

    def _length_of(self, ids):
        return max(1, min(self.max_len, len(ids)))

    def load_length(self, filepath):
        """-> the song's length in [1, max_len]: the length sidecar; max_len for a token sidecar that has none; else the song is
        tokenised (and, with persist, both sidecars are written)."""
        side = self.length_sidecar_path(filepath)
        if self.persist and os.path.isfile(side):
            return int(np.load(side).reshape(-1)[0])
        if self.persist and os.path.isfile(self.sidecar_path(filepath)):
            return self.max_len
        if self.persist:
            self.load(filepath)
            return int(np.load(side).reshape(-1)[0])
        return self._length_of(self.tokenize(self.read(filepath)))

    def validate(self, filepath):
        """A song is valid iff it loads (base_loader.py:35-50)."""
        try:
            self.load(filepath)
        except _VALIDATION_ERRORS:
            return False
        return True

    def load(self, filepath):
        """-> int32 [max_len] (base_loader.py:52-64)."""
        sidecar = self.sidecar_path(filepath)
        if self.persist and os.path.isfile(sidecar):
            return np.load(sidecar).astype(self.dtype)
        ids = self.tokenize(self.read(filepath))
        row = np.zeros(self.max_len, dtype=self.dtype)
        n = min(self.max_len, len(ids))
        row[:n] = ids[:n]
        if self.persist:
            # the length first: a token sidecar without a length sidecar reads as "max_len"
            self._save_atomically(self.length_sidecar_path(filepath), np.array([self._length_of(ids)], np.int32))
            self._save_atomically(sidecar, row)
        return row
