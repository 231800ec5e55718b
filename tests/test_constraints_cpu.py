"""Constrained decoding without a GPU: data.constraints (the Constraints class and the MIDI preset) and the fp64
restatement tests/constraint_ref.py -- the MIDI preset's properties on random and on decoded streams, the golden songs that pin
why the preset is no tokenizer grammar, an fp32 stand-in of the device's decoder through the margin check at the GPU tests'
shapes, and seven planted mistakes that the checks must catch."""
import json
import os

import numpy as np
import pytest

import constraint_ref as CR
from conftest import small_config
from data import midi_loader as M
from data.constraints import Constraints, midi_constraints
from oracle import lstm_oracle as O

V = M.OFF_TIME + M.MAX_SHIFT_STEPS          # 4708


# -------------------------------------------------------------------------------- the Constraints class
def test_constraints_allowed_advance_and_refusals():
    con = Constraints(6, bias=[0, 0, -np.inf, 0, 0, 0], token_class=[0, 0, 0, 1, 1, 0], next_state=[[0, 1], [0, -1]],
                      slot_open=[0, -1, -1, -1, -1, 33], slot_close=[-1, 0, -1, -1, 33, -1], n_slots=34)
    s, o = con.initial()
    assert o.shape == (2,) and con.allowed(s, o).tolist() == [True, False, False, True, False, True]
    s, o = con.advance(s, o, 5)                     # opens slot 33: bit 1 of word 1
    assert o.tolist() == [0, 2] and s == 0
    s, o = con.advance(s, o, 3)                     # class 1: state 1, where class 1 is forbidden
    assert s == 1 and con.allowed(s, o).tolist() == [True, False, False, False, False, False]
    assert con.first_violation([5, 3, 4]) == 2 and con.first_violation([5, 4, 0, 1, 3, 0]) is None
    assert con.first_violation([2]) == 0 and con.first_violation([6]) == 0
    for bad in (dict(bias=[np.nan] + [0] * 5), dict(bias=[np.inf] + [0] * 5), dict(token_class=[0] * 6),
                dict(token_class=[0] * 5 + [2], next_state=[[0, 0]]), dict(token_class=[0] * 6, next_state=[[1]]),
                dict(token_class=[0] * 6, next_state=[[-2]]), dict(slot_open=[0] + [-1] * 5, n_slots=0),
                dict(slot_open=[0] + [-1] * 5, slot_close=[0] + [-1] * 5, n_slots=1), dict(n_slots=4097),
                dict(token_class=[0] * 6, next_state=np.zeros((257, 1), int)), dict(token_class=[0] * 6, next_state=np.zeros((1, 65), int)),
                dict(token_class=[0] * 6, next_state=[[0]], start_state=1)):
        with pytest.raises(ValueError):
            Constraints(6, **bad)


# -------------------------------------------------------------------------------- the MIDI preset
def _is(tok, lo, hi):
    return lo <= tok < hi


def _check_midi_stream(con, tokens, max_silence=None, instruments=None):
    tokens = [int(w) for w in tokens]
    assert con.first_violation(tokens) is None
    song = M.detokenize_tokens(tokens)
    n_off = sum(_is(w, M.OFF_NOTE_OFF, M.OFF_VELOCITY) for w in tokens)
    assert sum(len(notes) for _, notes in song.instruments) == n_off
    assert V not in tokens and max(tokens) < V
    if max_silence is not None:
        run = longest = 0
        for w in tokens:
            run = run + 1 if w >= M.OFF_TIME else 0
            longest = max(longest, run)
        assert longest <= max_silence
    if instruments is not None:
        for w in tokens:
            if w < M.OFF_NOTE_OFF:
                assert w // M.NUM_PITCHES in instruments
            elif _is(w, M.OFF_VELOCITY, M.OFF_TIME):
                assert (w - M.OFF_VELOCITY) // M.NUM_VELOCITY_BINS in instruments


@pytest.mark.parametrize('kw', [dict(), dict(max_silence=2), dict(instruments={0, 5}), dict(instruments={3}, max_silence=1)])
def test_midi_preset_on_random_streams(kw):
    """random id streams, each id drawn uniformly from the allowed set: what the preset lets through is what the detokenizer keeps"""
    con = midi_constraints(**kw)
    assert con.n_columns == V + 1 and con.n_slots == 2048
    rs = np.random.RandomState(3)
    for _ in range(3):
        s, o = con.initial()
        tokens = []
        for _ in range(400):
            ok = np.flatnonzero(con.allowed(s, o))
            assert ok.size > 0                      # the preset has no dead end: a note-on of an allowed family is always there ...
            # (close tokens drawn half of the time once notes sound, so that notes end as well as start)
            offs = ok[(ok >= M.OFF_NOTE_OFF) & (ok < M.OFF_VELOCITY)]
            w = int(rs.choice(offs)) if offs.size and rs.rand() < 0.5 else int(rs.choice(ok))
            tokens.append(w)
            s, o = con.advance(s, o, w)
        _check_midi_stream(con, tokens, **kw)
    # and a uniformly random id stream does break it, at once
    assert con.first_violation(rs.randint(0, V, size=64)) is not None


@pytest.mark.parametrize('kw', [dict(), dict(max_silence=3, instruments={0, 1, 2})])
def test_midi_preset_on_decoded_streams(kw):
    """streams drawn by the fp64 decoder under the preset, filters on"""
    cfg = small_config(input_size=V, max_len=8, embedding_size=4, hidden_size=8)
    params = O.glorot_init(cfg, 5)
    params['softmax_b'] = params['softmax_b'] + 2.0 * (np.arange(V + 1) >= M.OFF_NOTE_OFF)      # (note-offs and time shifts likely)
    con = midi_constraints(**kw)
    toks, _, cs = CR.generate(params, cfg, con, 2, 48, temperature=1.5, top_k=0, seed=4, top_p=0.95, theta=1.2, window=8)
    assert np.all(cs['dead_ends'] == 0)
    for row in toks:
        _check_midi_stream(con, row, **kw)
    # without the constraint the same model draws what the detokenizer drops
    free = Constraints(V + 1)
    toks, _, _ = CR.generate(params, cfg, free, 2, 48, temperature=1.5, seed=4, top_p=0.95, theta=1.2, window=8)
    assert any(con.first_violation(row) is not None for row in toks)


def test_golden_songs_pin_why_the_preset_is_no_tokenizer_grammar(golden_dir):
    """The grammar "a velocity is followed by a note-on of its family; a note-off only for a sounding note; no note-on for a sounding
    note" over the 25 tokenised golden songs: four break it within their first tokens (velocity bin 32 spills into the next
    family's bin 0; note-offs whose note-on never appears).  The preset -- what the detokenizer keeps -- has no velocity rule, so
    it reports only the three songs with such note-offs, which the detokenizer indeed drops."""
    songs = [s['tokens'] for s in json.load(open(os.path.join(golden_dir, 'g5_midi.json')))['tokenize']]
    assert len(songs) == 25
    F16, V1 = M.NUM_FAMILIES, V + 1
    cls = np.zeros(V1, np.int32)
    nxt = np.full((1 + F16, 1 + 2 * F16), -1, np.int32)
    nxt[0, :1 + F16] = 0                                   # free: anything but ...
    for f in range(F16):
        cls[f * M.NUM_PITCHES:(f + 1) * M.NUM_PITCHES] = 1 + f
        cls[M.OFF_VELOCITY + f * M.NUM_VELOCITY_BINS:M.OFF_VELOCITY + (f + 1) * M.NUM_VELOCITY_BINS] = 1 + F16 + f
        nxt[0, 1 + F16 + f] = 1 + f                        # ... a velocity of family f, which wants
        nxt[1 + f, 1 + f] = 0                              # a note-on of family f next
    preset = midi_constraints()
    grammar = Constraints(V1, token_class=cls, next_state=nxt, slot_open=preset.slot_open, slot_close=preset.slot_close, n_slots=2048)
    broken = [i for i, s in enumerate(songs) if grammar.first_violation(s) is not None]
    assert broken == [3, 6, 8, 17]
    assert all(grammar.first_violation(songs[i]) < 16 for i in broken)
    kept = [i for i, s in enumerate(songs) if preset.first_violation(s) is not None]
    assert kept == [3, 6, 8]
    for i, s in enumerate(songs):
        n_off = sum(_is(w, M.OFF_NOTE_OFF, M.OFF_VELOCITY) for w in s)
        n_notes = sum(len(notes) for _, notes in M.detokenize_tokens(s).instruments)
        assert (n_notes < n_off) == (i in kept), i


# -------------------------------------------------------------------------------- the fp32 stand-in at the GPU tests' shapes
@pytest.mark.parametrize('H,L', [(24, 1), (200, 2), (512, 1), (1024, 2)])
def test_fp32_stand_in_passes_the_margin_check(H, L):
    """tests/test_gpu_constraints.py::test_margins_across_hidden_sizes with an fp32 numpy decoder in the GPU's place: the margin
    check passes, and skips no more near-tie positions than test_generate_filters.py allows at these shapes (near <= 3)"""
    cfg = small_config(input_size=300, max_len=16, embedding_size=20, hidden_size=H, n_layers=L)
    params = O.glorot_init(cfg, 3)
    con = CR.mixed_constraint(301, K=33, seed=H)
    fk = dict(top_p=0.8, min_p=0.02, theta=1.5, window=0)
    toks, lps, cs = CR.generate(params, cfg, con, 5, 10, temperature=1.0, top_k=0, seed=11, dtype=np.float32, **fk)
    near = CR.check_margins(params, cfg, con, toks, lps, 1.0, 0, 11, cstate_out=cs, **fk)
    assert near <= 3
    primer = CR.allowed_primer(con, 5, 6, seed=1)
    toks, lps, cs = CR.generate(params, cfg, con, 5, 8, temperature=0.7, top_k=20, seed=12, primer=primer, dtype=np.float32, **fk)
    CR.check_margins(params, cfg, con, toks, lps, 0.7, 20, 12, primer=primer, cstate_out=cs, **fk)


# -------------------------------------------------------------------------------- planted mistakes
def _scenario():
    """bias, automaton and slots with every filter on, slot 32 in play and a primer that opens slots"""
    cfg = small_config(input_size=79, max_len=8, embedding_size=6, hidden_size=12)
    params = O.glorot_init(cfg, 2)
    con = CR.mixed_constraint(80, K=36, seed=1, ban=0.05)
    con.bias[64] = 3.0          # the opener of slot 32 and its closer: likely draws
    con.bias[65] = 3.0
    primer = CR.allowed_primer(con, 4, 5, seed=2)
    return cfg, params, con, primer, dict(temperature=1.0, top_k=6, seed=9, top_p=0.9, min_p=0.02, theta=1.6, window=0)


def _dead_end_scenario():
    """every column opens a slot of its own: after V1 draws nothing is allowed any more"""
    cfg = small_config(input_size=11, max_len=8, embedding_size=4, hidden_size=8)
    con = Constraints(12, slot_open=np.arange(12), n_slots=12)
    return cfg, O.glorot_init(cfg, 4), con, None, dict(temperature=1.0, top_k=0, seed=3, top_p=0.0, min_p=0.0, theta=1.0, window=0)


def _run(scenario, mistake, num):
    cfg, params, con, primer, kw = scenario
    toks, lps, cs = CR.generate(params, cfg, con, 4, num, primer=primer, mistake=mistake, **kw)
    return CR.check_margins(params, cfg, con, toks, lps, kw['temperature'], kw['top_k'], kw['seed'], top_p=kw['top_p'], min_p=kw['min_p'],
                            theta=kw['theta'], window=kw['window'], primer=primer, cstate_out=cs), toks, cs


def test_the_unplanted_decoder_passes():
    _, toks, cs = _run(_scenario(), None, 24)
    assert 64 in toks and 65 in toks                # slot 32 was opened and closed
    _, toks, cs = _run(_dead_end_scenario(), None, 16)
    assert cs['dead_ends'].tolist() == [4, 4, 4, 4] and all(sorted(r[:12]) == list(range(12)) for r in toks.tolist())


@pytest.mark.parametrize('mistake', CR.MISTAKES)
def test_planted_mistakes_fail_the_checks(mistake):
    scenario, num = (_dead_end_scenario(), 16) if mistake == 'dead_end_advances' else (_scenario(), 24)
    with pytest.raises(AssertionError):
        _run(scenario, mistake, num)


# -------------------------------------------------------------------------------- the train entry's key
def test_sample_constraints_key():
    """model YAML key sample_constraints: none (default: nothing passed on) | loader (the loader's constraints, if it has any)"""
    import train.train as T
    from data.base_loader import Loader
    from data.midi_loader import MIDILoader

    class Sampler(object):
        def __init__(self, loader):
            self.loader = loader

        def constraints(self, **kw):
            return self.loader.constraints(**kw)

    midi, plain = Sampler(MIDILoader(8, persist=False)), Sampler(Loader(8, persist=False))
    assert T.sample_constraints({}, midi) == {} and T.sample_constraints({'sample_constraints': 'none'}, midi) == {}
    assert T.sample_constraints({'sample_constraints': None}, midi) == {}
    got = T.sample_constraints({'sample_constraints': 'loader'}, midi)
    assert list(got) == ['constraints'] and got['constraints'].n_columns == V + 1 and got['constraints'].n_slots == 2048
    assert T.sample_constraints({'sample_constraints': 'loader'}, plain) == {}
    with pytest.raises(ValueError):
        T.sample_constraints({'sample_constraints': 'grammar'}, midi)
