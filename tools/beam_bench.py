#!/usr/bin/env python3
"""Per-position time of fsmg_beam_search (batched on-device beam search) at cfg-B and cfg-C dims against fsmg_generate at
temperature 0 with B = G * W rows on the same handle, the two calls alternating within each repetition.  Prints one line per case
and one JSON line per case (--json FILE also writes them to a file).

  python tools/beam_bench.py [--num 256] [--reps 5] [--configs cfg-B,cfg-C] [--cases 1x1,1x8,4x16,16x4,1x64] [--json FILE]

us/position = wall time of one call (median of --reps after one warm-up call of each) / num; hypotheses*tokens/s = G * W * num /
wall time.  Every call ends in its device-to-host copy, so the wall time covers the device work."""
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


def alternating_medians(fns, reps):
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            ts[i].append(time.perf_counter() - t0)
    return [float(np.median(t)) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='cfg-B,cfg-C')
    ap.add_argument('--num', type=int, default=256)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--cases', default='1x1,1x8,4x16,16x4,1x64', help='GxW list')
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    from fsmg.binding import FsmgModel
    rows = []
    num = args.num
    for name in args.configs.split(','):
        cfg = dict(CONFIGS[name], name='lstm_baseline', seed=1, max_len=128, lr=1e-3, max_grad_norm=5, n_decay=1000)
        m = FsmgModel(cfg)
        m.init_params(1)
        for case in args.cases.split(','):
            G, W = [int(x) for x in case.split('x')]
            B = G * W
            tb, tg = alternating_medians([lambda: m.beam_search(num, W, n_groups=G),
                                          lambda: m.generate(B, num, temperature=0.0)], args.reps)
            r = dict(config=name, n_groups=G, beam_width=W, rows=B, num=num, beam_seconds=tb, beam_us_per_position=1e6 * tb / num,
                     beam_hyp_tokens_per_s=B * num / tb, generate_seconds=tg, generate_us_per_position=1e6 * tg / num,
                     generate_tokens_per_s=B * num / tg, beam_over_generate=tb / tg)
            rows.append(r)
            print('%s G=%-3d W=%-3d (B=%-3d): beam %8.2f us/position %10.0f hyp*tok/s | generate T=0 %8.2f us/position | %.2fx'
                  % (name, G, W, B, r['beam_us_per_position'], r['beam_hyp_tokens_per_s'], r['generate_us_per_position'],
                     r['beam_over_generate']))
        m.close()
    for r in rows:
        print(json.dumps(r))
    if args.json:
        with open(args.json, 'w') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
