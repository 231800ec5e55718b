#!/usr/bin/env python3
"""Per-position time of fsmg_cache_generate (every generated token drawn from the support-set mixture) against fsmg_generate at the
same rows, seed and temperature on the same handle, at cfg-B dims, the two calls alternating within each repetition; and the two
cache kernels' own times per position (event timing, one kernel class at a time).  Prints one line per shape and one JSON line per
shape (--json FILE also writes them to a file).

  python tools/cachegen_bench.py [--num 128] [--reps 7] [--shapes 25x5x640,64x1x25600] [--theta 1.0] [--lam 0.25] [--json FILE]

A shape is rows x groups x entries-per-group; row r attends over group r % groups.  us/position = wall time of one call (median of
--reps after one warm-up call of each) / num.  Every call ends in its device-to-host copy, so the wall time covers the device work.
The keys are random vectors of the size of hidden states; the time does not depend on their values."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'few-shot-music-generation_amd', 'src'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np          # noqa: E402
from beam_bench import CONFIGS, alternating_medians     # noqa: E402


def kernel_us(m, kernel_class, call):
    """device time of one kernel class per launch, in microseconds, over one call"""
    m.timing_enable(True)
    m.timing_select(kernel_class)
    m.timing_reset()
    call()
    ms, n = m.timing_read(kernel_class)
    m.timing_select(None)
    m.timing_enable(False)
    return 1e3 * ms / max(n, 1), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='cfg-B')
    ap.add_argument('--num', type=int, default=128)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--shapes', default='25x5x640,64x1x25600')
    ap.add_argument('--temperature', type=float, default=1.0)
    ap.add_argument('--theta', type=float, default=1.0)
    ap.add_argument('--lam', type=float, default=0.25)
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    from fsmg.binding import FsmgModel
    cfg = dict(CONFIGS[args.config], name='lstm_baseline', seed=1, max_len=128, lr=1e-3, max_grad_norm=5, n_decay=1000)
    m = FsmgModel(cfg)
    m.init_params(1)
    H, V = cfg['hidden_size'], cfg['input_size']
    num, T = args.num, args.temperature
    rows = []
    for shape in args.shapes.split(','):
        R, G, Mg = [int(x) for x in shape.split('x')]
        rng = np.random.RandomState(R)
        cache = m.cache_from(rng.uniform(-0.5, 0.5, size=(G, Mg, H)).astype(np.float32), rng.randint(0, V, size=(G, Mg)).astype(np.int32))
        group = (np.arange(R) % G).astype(np.int32)

        def mixed():
            return m.cache_generate(cache, R, num, args.theta, args.lam, group=group, temperature=T, seed=3)

        tc, tg = alternating_medians([mixed, lambda: m.generate(R, num, temperature=T, seed=3)], args.reps)
        scores_us, n_scores = kernel_us(m, 'cache_scores', mixed)
        mix_us, n_mix = kernel_us(m, 'cache_mix', mixed)
        assert n_scores == num and n_mix == num, (n_scores, n_mix)
        cache.close()
        r = dict(config=args.config, rows=R, groups=G, entries_per_group=Mg, num=num, temperature=T, theta=args.theta, lam=args.lam,
                 cache_generate_seconds=tc, cache_generate_us_per_position=1e6 * tc / num, generate_seconds=tg,
                 generate_us_per_position=1e6 * tg / num, cache_over_generate=tc / tg, cache_scores_us=scores_us, cache_mix_us=mix_us)
        rows.append(r)
        print('%s %d rows, %d x %d entries: cache_generate %8.2f us/position | generate %8.2f us/position | %.2fx | k_cache_scores '
              '%.2f us, k_cache_mix %.2f us' % (args.config, R, G, Mg, r['cache_generate_us_per_position'], r['generate_us_per_position'],
                                               r['cache_over_generate'], scores_us, mix_us))
    m.close()
    for r in rows:
        print(json.dumps(r))
    if args.json:
        with open(args.json, 'w') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
