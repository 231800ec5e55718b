"""The padding-masked loss without a GPU: the fp64 restatement (tests/masked_ref.py) against the oracle at full lengths and
against an independent torch-autograd masked loss, its padding law, the new entry points' refusals that need no device, and the
lengths' way from the loader's sidecar through the dataset, the sampler and train.train to the plugin."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import yaml

import masked_ref as MR
from conftest import ROOT, small_config
from oracle import lstm_oracle as O

MASKED_ENTRY_POINTS = ('fsmg_train_step_masked', 'fsmg_forward_backward_masked', 'fsmg_eval_step_masked', 'fsmg_eval_batch_masked',
                       'fsmg_upload_table_lengths', 'fsmg_train_step_indexed_masked', 'fsmg_forward_backward_indexed_masked')


def _case(cfg, N, K, Q, seed):
    (sup, qry), = O.synthetic_episodes(1, N, K, Q, cfg['max_len'], cfg['input_size'], seed=seed)
    rng = np.random.RandomState(seed + 50)
    sl, ql = MR.lengths_for(rng, (N, K), cfg['max_len']), MR.lengths_for(rng, (N, Q), cfg['max_len'])
    return sup, qry, sl, ql, rng


@pytest.mark.parametrize('over', [dict(), dict(n_layers=2, hidden_size=12)])
def test_full_lengths_are_the_oracle_bit_for_bit(over):
    cfg = small_config(**over)
    sup, qry, sl, ql, _ = _case(cfg, 2, 2, 1, 3)
    params = O.glorot_init(cfg, 7)
    X, Y = O.train_xy(sup, qry, cfg['input_size'])
    loss, cache = O.forward(params, X, Y, cfg)
    grads, aux = O.backward(params, cache, cfg)
    T = cfg['max_len']
    mloss, _, mgrads, maux = MR.step(params, sup, qry, np.full_like(sl, T), np.full_like(ql, T), cfg)
    assert mloss == float(loss) and maux == aux
    for k in grads:
        assert np.array_equal(grads[k].view(np.uint64), mgrads[k].view(np.uint64)), k
    assert MR.eval_step(params, qry, np.full_like(ql, T), cfg) == O.eval_step(params, qry, cfg)


def _torch_masked(params, X, Y, lengths, cfg):
    """an independent statement: torch autograd of the masked mean of F.cross_entropy over an LSTM written with torch ops, fp64"""
    import torch
    import torch.nn.functional as F
    d = O.model_dims(cfg)
    H, L, T = d['H'], d['L'], d['T']
    p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    x = p['embedding'][torch.tensor(X, dtype=torch.long)]              # [B, T, E]
    B = x.shape[0]
    for l in range(L):
        K, b = p['kernel_%d' % l], p['bias_%d' % l]
        h = torch.zeros(B, H, dtype=torch.float64)
        c = torch.zeros(B, H, dtype=torch.float64)
        outs = []
        for t in range(T):
            z = torch.cat([x[:, t], h], dim=1) @ K + b
            i, j, f, o = z.split(H, dim=1)
            c = c * torch.sigmoid(f + O.FORGET_BIAS) + torch.sigmoid(i) * torch.tanh(j)
            h = torch.tanh(c) * torch.sigmoid(o)
            outs.append(h)
        x = torch.stack(outs, dim=1)
    logits = x.reshape(B * T, H) @ p['softmax_w'] + p['softmax_b']
    ce = F.cross_entropy(logits, torch.tensor(Y.reshape(-1), dtype=torch.long), reduction='none')
    mask = torch.tensor((np.arange(T)[None, :] < np.asarray(lengths)[:, None]).reshape(-1))
    loss = ce[mask].sum() / (float(np.sum(lengths)) + 1e-12)
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in p.items()}


@pytest.mark.parametrize('over', [dict(), dict(n_layers=2, hidden_size=12)])
def test_random_lengths_against_torch_autograd(over):
    """1e-9: the bound the MAML oracle is held to against autograd (DESIGN.md "cfg-E")"""
    cfg = small_config(**over)
    sup, qry, sl, ql, _ = _case(cfg, 3, 2, 2, 4)
    params = O.glorot_init(cfg, 8)
    loss, cache, grads, _ = MR.step(params, sup, qry, sl, ql, cfg)
    X, Y = O.train_xy(sup, qry, cfg['input_size'])
    want_loss, want = _torch_masked(params, X, Y, MR.train_lengths(sl, ql), cfg)
    assert abs(loss - want_loss) <= 1e-9
    for k in grads:
        assert np.abs(grads[k] - want[k]).max() <= 1e-9 * max(1.0, np.abs(want[k]).max()), k
    # and the mask does something: the unmasked loss of the same episode is another number
    assert abs(float(O.forward(params, X, Y, cfg, keep=False)[0]) - loss) > 1e-6


def test_padding_never_matters_in_the_restatement():
    cfg = small_config()
    sup, qry, sl, ql, rng = _case(cfg, 2, 2, 2, 5)
    params = O.glorot_init(cfg, 9)
    sup2, qry2 = MR.scramble_padding(sup, sl, cfg['input_size'], rng), MR.scramble_padding(qry, ql, cfg['input_size'], rng)
    assert not np.array_equal(sup, sup2) and not np.array_equal(qry, qry2)
    assert np.array_equal(sup[0, 0, :sl[0, 0]], sup2[0, 0, :sl[0, 0]])
    a, b = MR.step(params, sup, qry, sl, ql, cfg), MR.step(params, sup2, qry2, sl, ql, cfg)
    assert a[0] == b[0] and a[3] == b[3]
    for k in a[2]:
        assert np.array_equal(a[2][k], b[2][k]), k
    assert MR.eval_step(params, qry, ql, cfg) == MR.eval_step(params, qry2, ql, cfg)


# ----------------------------------------------------------------------------- the C-ABI, before any device
def test_entry_points_are_declared_bound_exported_and_refuse_bad_arguments():
    from fsmg.build import build
    build()
    from fsmg import binding as B
    out = subprocess.check_output(['nm', '-D', '--defined-only', B.library_path()], universal_newlines=True)
    text = open(os.path.join(ROOT, 'include', 'fsmg.h')).read()
    for name in MASKED_ENTRY_POINTS:
        assert name in B.SIGNATURES and re.search(r' T %s$' % name, out, flags=re.M) and re.search(r'\bint %s\(' % name, text), name
        assert re.fullmatch(r'fsmg_[a-z_]+', name)
    assert int(re.search(r'#define FSMG_VERSION (\d+)', text).group(1)) == 600
    assert int(re.search(r'#define FSMG_CONFIG_VERSION (\d+)', text).group(1)) == 4
    blob = open(B.library_path(), 'rb').read().decode('latin-1')
    for kernel in ('k_row_weights', 'k_ce_finish_w', 'k_ce_rows_w', 'k_ce_rows_reg_w', 'k_loss_reduce_w', 'k_gather_rows_len', 'k_token_prep_len'):
        assert kernel in blob, kernel
    lib = B.load_library()
    toks = np.zeros((4, 10), np.int32)
    lens = np.ones(4, np.int32)
    idx = np.zeros(4, np.int32)
    loss = C.c_float()
    nll = np.zeros(4, np.float32)
    tp, lp, ip = C.c_void_p(toks.ctypes.data), C.c_void_p(lens.ctypes.data), C.c_void_p(idx.ctypes.data)
    fp = nll.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.fsmg_train_step_masked(None, tp, tp, lp, lp, 1, 2, 2, 0, C.byref(loss)) == -1
    assert lib.fsmg_forward_backward_masked(None, tp, tp, lp, lp, 1, 2, 2, 0) == -1
    assert lib.fsmg_eval_step_masked(None, tp, lp, 2, 2, 0, fp) == -1
    assert lib.fsmg_eval_batch_masked(None, tp, lp, 1, 2, 2, 0, fp) == -1
    assert lib.fsmg_upload_table_lengths(None, 0, lp, 4) == -1
    assert lib.fsmg_train_step_indexed_masked(None, 0, ip, ip, 1, 2, 2, C.byref(loss)) == -1
    assert lib.fsmg_forward_backward_indexed_masked(None, 0, ip, ip, 1, 2, 2) == -1


def test_binding_checks_lengths_before_the_library():
    from fsmg.binding import FsmgModel
    lp = FsmgModel._len_ptr
    with pytest.raises(ValueError, match='needs lengths'):
        lp(None, 4, 0)
    with pytest.raises(ValueError, match='3 lengths for 4'):
        lp(np.ones(3, np.int32), 4, 0)
    with pytest.raises(ValueError, match='one flag'):
        lp(np.ones(4, np.int32), 4, 1)
    with pytest.raises(ValueError, match='one flag'):
        lp(12345, 4, 0)
    ptr, keep = lp(np.ones((2, 2), np.int64), 4, 0)
    assert keep.dtype == np.int32 and keep.shape == (4,) and ptr.value == keep.ctypes.data


# ----------------------------------------------------------------------------- loader, sidecars, dataset, sampler
T, K, Q = 32, 5, 4


def _raw_tree(tmp_path, golden_dir):
    dst = tmp_path / 'raw'
    shutil.copytree(os.path.join(golden_dir, 'g1_lyrics'), dst, ignore=shutil.ignore_patterns('*.npy', 'few_shot_metadata_*'))
    return str(dst)


def _dataset(root, split='train'):
    from data.dataset import Dataset, Metadata
    from data.lyrics_loader import LyricsLoader
    md = Metadata(root, 'few_shot_metadata_lyrics_%d' % T)
    loader = LyricsLoader(T, metadata=md, tokenizer=str.split)
    return Dataset(root, split, loader, md, min_songs=K + Q, seed=0), loader


def test_length_sidecar_is_written_and_read(tmp_path, golden_dir):
    root = _raw_tree(tmp_path, golden_dir)
    ds, loader = _dataset(root)
    table, offsets = ds.token_table()
    lengths = ds.length_table()
    assert lengths.dtype == np.int32 and lengths.shape == (table.shape[0],) and lengths.min() >= 1 and lengths.max() <= T
    assert (lengths < T).any() and (lengths == T).any(), 'the fixture holds short and full songs'
    row = 0
    for artist in ds.artists:                                  # the order of token_table(): artist by artist, artist.songs order
        for song in artist.songs:
            path = os.path.join(root, artist.name, song)
            n_words = len(open(path).read().split())
            assert lengths[row] == max(1, min(T, n_words)), path
            side = path + '.%d.len.npy' % T
            assert side == loader.length_sidecar_path(path) and os.path.isfile(side)
            on_disk = np.load(side)
            assert on_disk.dtype == np.int32 and on_disk.shape == (1,) and on_disk[0] == lengths[row]
            assert loader.load_length(path) == lengths[row]
            assert (table[row, lengths[row]:] == 0).all()
            row += 1
    assert row == table.shape[0] == offsets[-1]
    assert not [f for a in ds.artists for f in os.listdir(os.path.join(root, a.name)) if '.tmp.' in f]     # written atomically
    # a second dataset over the same tree reads the sidecars back
    again, _ = _dataset(root)
    assert np.array_equal(again.length_table(), lengths)


def test_a_token_sidecar_without_a_length_sidecar_means_max_len(tmp_path, golden_dir):
    """the case of a tree the reference wrote (the golden fixture is one): nothing is guessed from zeros"""
    root = str(tmp_path / 'g1_lyrics')
    shutil.copytree(os.path.join(golden_dir, 'g1_lyrics'), root)
    from data.episode import load_sampler_from_config
    sampler = load_sampler_from_config(dict(dataset='lyrics', dataset_path=root, max_len=T, query_size=Q, support_size=K,
                                            batch_size=2, seed=1234, split='train'))
    table = sampler.token_table()
    assert (table == 0).any()
    lengths = sampler.length_table()
    assert lengths.shape == (table.shape[0],) and (lengths == T).all()
    assert not [f for d, _, fs in os.walk(root) for f in fs if f.endswith('.len.npy')]


def test_episode_lengths_agree_with_the_table_and_the_stream_is_unchanged(tmp_path, golden_dir):
    from data.episode import Episode, EpisodeSampler
    root = _raw_tree(tmp_path, golden_dir)
    ds, _ = _dataset(root)
    lengths = ds.length_table()
    a = EpisodeSampler(ds, 2, K, Q, T, seed=99)

    class NoLengths(object):                                   # the same split through a dataset that keeps no lengths
        def __init__(self, inner):
            self.inner, self.loader = inner, inner.loader

        def token_table(self):
            return self.inner.token_table()

        def __len__(self):
            return len(self.inner)

    b = EpisodeSampler(NoLengths(ds), 2, K, Q, T, seed=99)
    for _ in range(5):
        si, qi = a.episode_indices()
        ep = a.gather(si, qi)
        assert ep.support_len.dtype == np.int32 and ep.support_len.shape == (2, K) and ep.query_len.shape == (2, Q)
        assert np.array_equal(ep.support_len, lengths[si]) and np.array_equal(ep.query_len, lengths[qi])
        other = b.get_episode()
        assert other.support_len is None and other.query_len is None
        assert np.array_equal(other.support, ep.support) and np.array_equal(other.query, ep.query)
    by_hand = Episode(ep.support, ep.query)
    assert by_hand.support_len is None and by_hand.query_len is None


# ----------------------------------------------------------------------------- train.train and the plugins
class _Recorder(object):
    """a plugin of the test's own with the fast path's members: records what train.train hands to attach_table"""
    calls = []

    def __init__(self, config):
        self.mask_padding = bool(config.get('mask_padding', False))
        self._config = config
        _Recorder.calls = []

    def recover_or_init(self, init_path):
        pass

    def attach_table(self, split, table, lengths=None):
        _Recorder.calls.append(('attach_table', split, table.shape, None if lengths is None else np.array(lengths)))

    def train_indexed(self, split, support_idx, query_idx, want_loss=False):
        _Recorder.calls.append(('train_indexed', split))

    def recent_losses(self, n):
        return [1.0] * n

    def train(self, episode):
        return 1.0

    def eval(self, episode):
        _Recorder.calls.append(('eval', None if episode.query_len is None else episode.query_len.shape))
        return 2.0

    def sample(self, support_set, num):
        return [0] * num

    def save(self, checkpt_path):
        pass


@pytest.mark.parametrize('mask', [True, False])
def test_train_hands_the_lengths_to_attach_table(tmp_path, golden_dir, mask, monkeypatch):
    import train.train as TT
    monkeypatch.setitem(sys.modules, 'masked_recorder', sys.modules[__name__])
    monkeypatch.delenv('FSMG_TRAIN_SYNC', raising=False)
    root = _raw_tree(tmp_path, golden_dir)
    _dataset(root)[0].metadata.close()        # tokenise the tree once with the whitespace tokenizer: both sidecars of every song, vocabulary, splits
    docs = {
        'data': dict(dataset='lyrics', dataset_path=root, splits=['train', 'val', 'test'], max_len=T),
        'task': dict(query_size=Q, support_size=K, seed=1234),
        'model': dict(n_train=2, print_every_n=2, val_every_n=2.0, n_val=1, n_test=1, n_samples=0, batch_size=2, name='rec',
                      model_module_name='masked_recorder', model_class_name='_Recorder', mask_padding=mask),
    }
    paths = {}
    for name, doc in docs.items():
        paths[name] = str(tmp_path / (name + '.yaml'))
        with open(paths[name], 'w') as f:
            yaml.safe_dump(doc, f)
    TT.main(['--data', paths['data'], '--task', paths['task'], '--model', paths['model']])
    attach = [c for c in _Recorder.calls if c[0] == 'attach_table']
    assert len(attach) == 1 and attach[0][1] == 'train'
    n_songs = attach[0][2][0]
    if mask:
        lengths = attach[0][3]
        assert lengths.shape == (n_songs,) and lengths.dtype == np.int32 and (lengths < T).any() and lengths.min() >= 1
    else:
        assert attach[0][3] is None                            # the old path: the table alone
    assert [c for c in _Recorder.calls if c[0] == 'train_indexed'] == [('train_indexed', 'train')] * 2
    assert ('eval', (2, Q)) in _Recorder.calls                # the validation episodes carry their lengths either way


def test_plugins_take_or_refuse_the_key_without_a_device():
    from models.cache_lstm import CacheLSTM
    from models.maml_lstm import MAMLLSTM
    cfg = dict(small_config(), mask_padding=True)
    with pytest.raises(RuntimeError, match='MAMLLSTM has no padding-masked loss'):
        MAMLLSTM(dict(cfg))
    with pytest.raises(RuntimeError, match='CacheLSTM has no padding-masked loss'):
        CacheLSTM(dict(cfg, cache_theta=1.0, cache_lambda=0.5))
    conf = os.path.join(ROOT, 'few-shot-music-generation_amd', 'src', 'config')
    masked = yaml.safe_load(open(os.path.join(conf, 'lstm_masked.yaml')))
    base = yaml.safe_load(open(os.path.join(conf, 'lstm_baseline.yaml')))
    assert masked['mask_padding'] is True and 'mask_padding' not in base
    assert masked['model_module_name'] == 'models.lstm_baseline' and masked['model_class_name'] == 'LSTMBaseline'
    assert {k: v for k, v in masked.items() if k not in ('name', 'mask_padding')} == {k: v for k, v in base.items() if k != 'name'}


def test_episode_parallel_passes_the_lengths_through():
    """fsmg.dist.EpisodeParallel with an engine of the test's own: the masked keyword reaches the engine's calls, an unmasked step
    hands it nothing"""
    from fsmg.dist import EpisodeParallel

    class Engine(object):
        def __init__(self, fused):
            self.calls = []
            if fused:
                self.fused_train_step = self._fused

        def _fused(self, support, query, want_loss=True, table=None, **kw):
            self.calls.append(('fused', table, kw))
            return 1.0

        def forward_backward(self, support, query, **kw):
            self.calls.append(('fb', kw))

        def forward_backward_indexed(self, table, support, query, **kw):
            self.calls.append(('fbi', table, kw))

        def apply_update(self, scale, want_loss=True):
            return 2.0

    lens = (np.ones((1, 1), np.int32), np.ones((1, 1), np.int32))
    for fused in (True, False):
        e = Engine(fused)
        p = EpisodeParallel(e)
        p.train_step('s', 'q')
        p.train_step('s', 'q', lengths=lens)
        p.train_step('s', 'q', table=0, lengths=True)
        if fused:
            assert e.calls == [('fused', None, {}), ('fused', None, {'lengths': lens}), ('fused', 0, {'lengths': True})]
        else:
            assert e.calls == [('fb', {}), ('fb', {'lengths': lens}), ('fbi', 0, {'lengths': True})]
        with pytest.raises(ValueError, match='MAML'):
            p.train_step('s', 'q', lengths=lens, maml=(1, 0.1))
