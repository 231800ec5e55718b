#!/usr/bin/env python3
"""Per-position time of fsmg_beam_search_constrained against fsmg_beam_search at the same (G, W): same handle, the legs alternating
within each repetition in one process -- unconstrained (A), unconstrained again (A', the A/A leg: the noise floor), constrained (C).
Prints one line and one JSON line per shape (--json FILE also appends them to a file).

  python tools/beamcon_bench.py [--num 128] [--reps 15] [--shapes midi-1x8,midi-4x16,midi-1x64,big-1x8,big-4x16,big-1x64] [--json FILE]
  python tools/beamcon_bench.py --trace-only --shapes midi-4x16      # the legs without timing, for a kernel trace of its own

us/position = wall time of one call (median of --reps after one warm-up call of each leg) / num.  Every call ends in its
device-to-host copy, so the wall time covers the device work.  aa_spread = |A' - A| / A; the constrained leg is slower than the
unconstrained one beyond the noise only where (C - A) / A exceeds it.

Shapes: midi-GxW: the MIDI vocabulary (V1 = 4709, the staged row kernel), hidden 1024 x 2, under the MIDI preset with
max_silence = 8; big-GxW: V1 = 50001 (the unstaged row kernel), hidden 1024 x 2, under tools/constrain_bench.py's big constraint
(a bias that bans a tenth of the columns, a 4-state automaton over 8 classes, 2048 slots)."""
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
from constrain_bench import big_constraint     # noqa: E402


def shape(name):
    kind, gw = name.split('-')
    G, W = (int(x) for x in gw.split('x'))
    from data.constraints import midi_constraints
    V1 = 4709 if kind == 'midi' else 50001
    cfg = dict(name='lstm_baseline', seed=1, input_size=V1 - 1, max_len=128, embedding_size=250, hidden_size=1024, n_layers=2, lr=1e-3,
               max_grad_norm=5, n_decay=1000)
    return cfg, G, W, (midi_constraints(max_silence=8) if kind == 'midi' else big_constraint(V1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='midi-1x8,midi-4x16,midi-1x64,big-1x8,big-4x16,big-1x64')
    ap.add_argument('--num', type=int, default=128)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--trace-only', action='store_true', help='run each leg --reps times without timing (for a kernel trace)')
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    from fsmg.binding import FsmgModel
    num = args.num
    out = []
    models = {}
    for name in args.shapes.split(','):
        cfg, G, W, con = shape(name)
        key = cfg['input_size']
        if key not in models:
            m = FsmgModel(cfg)
            m.init_params(1)
            models[key] = (m, m.new_constraint(con))
        m, dc = models[key]
        plain = lambda: m.beam_search(num, W, n_groups=G)
        constrained = lambda: m.beam_search(num, W, n_groups=G, constraints=dc, return_cstate=True)
        toks, scores, cs = constrained()
        assert con.first_violation(toks[0, 0]) is None and con.first_violation(toks[-1, -1]) is None
        if args.trace_only:
            for _ in range(args.reps):
                plain()
                constrained()
            continue
        ta, ta2, tc = alternating_medians([plain, plain, constrained], args.reps)
        r = dict(shape=name, V1=cfg['input_size'] + 1, hidden=cfg['hidden_size'], layers=cfg['n_layers'], groups=G, width=W, num=num,
                 reps=args.reps, beam_us_per_position=1e6 * ta / num, beam_again_us_per_position=1e6 * ta2 / num,
                 constrained_us_per_position=1e6 * tc / num, aa_spread=abs(ta2 - ta) / ta, constrained_over_beam=tc / ta,
                 dead_ends=int(np.sum(cs['dead_ends'])))
        out.append(r)
        print('%-10s V1=%-5d G=%-2d W=%-2d: beam %8.2f | again %8.2f (A/A %.2f %%) | constrained %8.2f us/position (%+.2f %%)'
              % (name, r['V1'], G, W, r['beam_us_per_position'], r['beam_again_us_per_position'], 100 * r['aa_spread'],
                 r['constrained_us_per_position'], 100 * (r['constrained_over_beam'] - 1)))
    for r in out:
        print(json.dumps(r))
    if args.json:
        with open(args.json, 'a') as f:
            for r in out:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
