#!/usr/bin/env python3
"""Per-position time of fsmg_generate_filtered (top-p, min-p, repetition penalty) against fsmg_generate at the same temperature and
top_k = 0 on the same handle, at cfg-B and cfg-C dims, the two calls alternating within each repetition.  Prints one line per case
and one JSON line per case (--json FILE also writes them to a file).

  python tools/filter_bench.py [--num 256] [--reps 5] [--configs cfg-B,cfg-C] [--batches 1,64,256] [--cases ...] [--json FILE]

us/position = wall time of one call (median of --reps after one warm-up call of each) / num.  Every call ends in its
device-to-host copy, so the wall time covers the device work.  Cases: neutral (filters all off: the fsmg_generate path),
top_p (0.9), min_p (0.05), penalty (1.2 over a window of 64), all (the three together)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'few-shot-music-generation_amd', 'src'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from beam_bench import CONFIGS, alternating_medians     # noqa: E402

CASES = {
    'neutral': dict(top_p=1.0, min_p=0.0, repetition_penalty=1.0),
    'top_p': dict(top_p=0.9),
    'min_p': dict(min_p=0.05),
    'penalty': dict(repetition_penalty=1.2, repeat_window=64),
    'all': dict(top_p=0.9, min_p=0.05, repetition_penalty=1.2, repeat_window=64),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='cfg-B,cfg-C')
    ap.add_argument('--num', type=int, default=256)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--batches', default='1,64,256')
    ap.add_argument('--cases', default=','.join(CASES))
    ap.add_argument('--temperature', type=float, default=1.0)
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    from fsmg.binding import FsmgModel
    rows = []
    num, T = args.num, args.temperature
    for name in args.configs.split(','):
        cfg = dict(CONFIGS[name], name='lstm_baseline', seed=1, max_len=128, lr=1e-3, max_grad_norm=5, n_decay=1000)
        m = FsmgModel(cfg)
        m.init_params(1)
        for B in [int(x) for x in args.batches.split(',')]:
            for case in args.cases.split(','):
                fk = CASES[case]
                tf, tg = alternating_medians([lambda: m.generate(B, num, temperature=T, seed=3, **fk),
                                              lambda: m.generate(B, num, temperature=T, seed=3)], args.reps)
                r = dict(config=name, rows=B, num=num, temperature=T, case=case, filters=fk, filtered_seconds=tf,
                         filtered_us_per_position=1e6 * tf / num, generate_seconds=tg, generate_us_per_position=1e6 * tg / num,
                         filtered_over_generate=tf / tg)
                rows.append(r)
                print('%s B=%-3d %-8s: filtered %8.2f us/position | generate %8.2f us/position | %.2fx'
                      % (name, B, case, r['filtered_us_per_position'], r['generate_us_per_position'], r['filtered_over_generate']))
        m.close()
    for r in rows:
        print(json.dumps(r))
    if args.json:
        with open(args.json, 'w') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
