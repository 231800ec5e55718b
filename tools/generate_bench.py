#!/usr/bin/env python3
"""Tokens/s of fsmg_generate (batched on-device sampling) at cfg-B and cfg-C dims against fsmg_sample (the same driver at one
greedy row) on the same handle.  Prints one line per case and one JSON line per case (--json FILE also writes them to a file).

  python tools/generate_bench.py [--num 256] [--reps 5] [--configs cfg-B,cfg-C] [--json profiles/generate_bench.jsonl]

tokens/s = n_seq * num / wall time of one call (median of --reps after one warm-up call); us/position = wall time / (P + num)
(primer positions run the cells only)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'few-shot-music-generation_amd', 'src'))
import numpy as np          # noqa: E402

CONFIGS = {
    'cfg-B': dict(input_size=10000, embedding_size=250, hidden_size=512, n_layers=1),
    'cfg-C': dict(input_size=4708, embedding_size=250, hidden_size=1024, n_layers=2),
}


def median_time(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='cfg-B,cfg-C')
    ap.add_argument('--num', type=int, default=256)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--batches', default='1,16,64,256')
    ap.add_argument('--primers', default='0,64')
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    from fsmg.binding import FsmgModel
    rows = []
    for name in args.configs.split(','):
        cfg = dict(CONFIGS[name], name='lstm_baseline', seed=1, max_len=128, lr=1e-3, max_grad_norm=5, n_decay=1000)
        m = FsmgModel(cfg)
        m.init_params(1)
        num = args.num
        t = median_time(lambda: m.sample(num), args.reps)
        base = dict(config=name, op='fsmg_sample', n_seq=1, num=num, primer_len=0, seconds=t, tokens_per_s=num / t,
                    us_per_position=1e6 * t / num)
        rows.append(base)
        print('%s fsmg_sample   B=1   P=0  : %10.0f tok/s  %7.2f us/position' % (name, base['tokens_per_s'], base['us_per_position']))
        rng = np.random.RandomState(0)
        for P in [int(p) for p in args.primers.split(',')]:
            for B in [int(b) for b in args.batches.split(',')]:
                primer = rng.randint(0, cfg['input_size'], size=(B, P)).astype(np.int32) if P else None
                t = median_time(lambda: m.generate(B, num, temperature=1.0, top_k=0, seed=3, primer=primer), args.reps)
                r = dict(config=name, op='fsmg_generate', n_seq=B, num=num, primer_len=P, seconds=t, tokens_per_s=B * num / t,
                         us_per_position=1e6 * t / (P + num), x_fsmg_sample=(B * num / t) / base['tokens_per_s'])
                rows.append(r)
                print('%s fsmg_generate B=%-4d P=%-3d: %10.0f tok/s  %7.2f us/position  %6.1fx fsmg_sample'
                      % (name, B, P, r['tokens_per_s'], r['us_per_position'], r['x_fsmg_sample']))
        m.close()
    for r in rows:
        print(json.dumps(r))
    if args.json:
        with open(args.json, 'w') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
