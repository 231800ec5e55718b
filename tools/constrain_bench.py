#!/usr/bin/env python3
"""Per-position time of fsmg_generate_constrained against fsmg_generate_filtered: same handle, rows, seed, temperature and filters,
the legs alternating within each repetition in one process -- filtered (A), filtered again (A', the A/A leg: the noise floor),
constrained (C).  Prints one line and one JSON line per shape (--json FILE also writes them to a file).

  python tools/constrain_bench.py [--num 128] [--reps 15] [--shapes midi-25,midi-64,big-25] [--filters all|none] [--json FILE]
  python tools/constrain_bench.py --trace-only --shapes midi-64      # the legs without timing, for a kernel trace of its own

us/position = wall time of one call (median of --reps after one warm-up call of each leg) / num.  Every call ends in its
device-to-host copy, so the wall time covers the device work.  aa_spread = |A' - A| / A; the constrained leg is slower than the
filtered one beyond the noise only where (C - A) / A exceeds it.  The pick kernels' own times come from a kernel trace of the
--trace-only run (profiles/README.md), not from this clock.

Shapes: midi-R: the MIDI vocabulary (V1 = 4709, the staged pick), hidden 1024 x 2, R rows, under the MIDI preset with
max_silence = 8; big-R: V1 = 50001 (the unstaged pick), hidden 1024 x 2, R rows, under a constraint with a bias that bans a tenth
of the columns, a 4-state automaton over 8 classes and 2048 slots."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'few-shot-music-generation_amd', 'src'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from beam_bench import alternating_medians     # noqa: E402

FILTERS = {'all': dict(top_p=0.9, min_p=0.05, repetition_penalty=1.2, repeat_window=64), 'none': {}}


def big_constraint(V1):
    from data.constraints import Constraints
    rs = np.random.RandomState(1)
    bias = np.where(rs.rand(V1) < 0.1, -np.inf, 0.0).astype(np.float32)
    bias[-1] = -np.inf
    token_class = rs.randint(0, 8, size=V1).astype(np.int32)
    next_state = rs.randint(0, 4, size=(4, 8)).astype(np.int32)
    next_state[np.arange(4), 1 + np.arange(4)] = -1
    K = 2048
    slot_open, slot_close = np.full(V1, -1, np.int32), np.full(V1, -1, np.int32)
    slot_open[:K], slot_close[K:2 * K] = np.arange(K), np.arange(K)
    return Constraints(V1, bias=bias, token_class=token_class, next_state=next_state, slot_open=slot_open, slot_close=slot_close, n_slots=K)


def shape(name):
    kind, rows = name.split('-')
    from data.constraints import midi_constraints
    V1 = 4709 if kind == 'midi' else 50001
    cfg = dict(name='lstm_baseline', seed=1, input_size=V1 - 1, max_len=128, embedding_size=250, hidden_size=1024, n_layers=2, lr=1e-3,
               max_grad_norm=5, n_decay=1000)
    return cfg, int(rows), (midi_constraints(max_silence=8) if kind == 'midi' else big_constraint(V1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='midi-25,midi-64,big-25')
    ap.add_argument('--num', type=int, default=128)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--filters', default='all', choices=sorted(FILTERS))
    ap.add_argument('--temperature', type=float, default=1.0)
    ap.add_argument('--trace-only', action='store_true', help='run each leg --reps times without timing (for a kernel trace)')
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    from fsmg.binding import FsmgModel
    num, T, fk = args.num, args.temperature, FILTERS[args.filters]
    out = []
    models = {}
    for name in args.shapes.split(','):
        cfg, B, con = shape(name)
        key = cfg['input_size']
        if key not in models:
            m = FsmgModel(cfg)
            m.init_params(1)
            models[key] = (m, m.new_constraint(con))
        m, dc = models[key]
        filtered = lambda: m.generate(B, num, temperature=T, seed=3, **fk)
        constrained = lambda: m.generate(B, num, temperature=T, seed=3, constraints=dc, return_cstate=True, **fk)
        toks, cs = constrained()
        assert con.first_violation(toks[0]) is None
        if args.trace_only:
            for _ in range(args.reps):
                filtered()
                constrained()
            continue
        ta, ta2, tc = alternating_medians([filtered, filtered, constrained], args.reps)
        r = dict(shape=name, V1=cfg['input_size'] + 1, hidden=cfg['hidden_size'], layers=cfg['n_layers'], rows=B, num=num, temperature=T,
                 filters=fk, reps=args.reps, filtered_us_per_position=1e6 * ta / num, filtered_again_us_per_position=1e6 * ta2 / num,
                 constrained_us_per_position=1e6 * tc / num, aa_spread=abs(ta2 - ta) / ta, constrained_over_filtered=tc / ta,
                 dead_ends=int(np.sum(cs['dead_ends'])))
        out.append(r)
        print('%-8s V1=%-5d B=%-3d filters=%-4s: filtered %8.2f | again %8.2f (A/A %.2f %%) | constrained %8.2f us/position (%+.2f %%)'
              % (name, r['V1'], B, args.filters, r['filtered_us_per_position'], r['filtered_again_us_per_position'], 100 * r['aa_spread'],
                 r['constrained_us_per_position'], 100 * (r['constrained_over_filtered'] - 1)))
    for r in out:
        print(json.dumps(r))
    if args.json:
        with open(args.json, 'a') as f:
            for r in out:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
