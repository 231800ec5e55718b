#!/usr/bin/env python3
"""Wall time per song of fsmg_cache_score against fsmg_score on the same rows and the same handle, the two calls alternating within
each repetition, and the attention kernel's own time and FLOP rate (the handle's event timers, class 'cache_attend', in a run of
their own).  Two shapes at cfg-B dims:

  episode   5 groups x 5 support songs, 5 query songs per group (one few-shot episode)
  large     1 group of 200 support songs, 640 query rows

  python tools/cache_bench.py [--reps 7] [--config cfg-B] [--max-len 128] [--thetas 1.0] [--json FILE]

us/song = wall time of one call (median of --reps after one warm-up call of each) / rows; every call ends in its device-to-host
copy.  Both calls ask for the row NLL and the per-token log-probs.  FLOP = 2 x queries x entries per group x hidden_size: the dot
products alone; the rate is set against the fp32 matrix pipe's 157.3 TFLOP/s and the fp64 pipe's 78.6 (the kernel runs on the
fp64 one)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'few-shot-music-generation_amd', 'src'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from beam_bench import CONFIGS, alternating_medians     # noqa: E402

PEAK_F32_MFMA, PEAK_F64_MFMA = 157.3e12, 78.6e12
SHAPES = {'episode': (5, 5, 5), 'large': (1, 200, 640)}          # groups, support songs per group, query songs per group


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='cfg-B')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--max-len', type=int, default=128)
    ap.add_argument('--shapes', default='episode,large')
    ap.add_argument('--thetas', default='1.0')
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    from fsmg.binding import FsmgModel
    T = args.max_len
    thetas = [float(x) for x in args.thetas.split(',')]
    cfg = dict(CONFIGS[args.config], name='lstm_baseline', seed=1, max_len=T, lr=1e-3, max_grad_norm=5, n_decay=1000)
    m = FsmgModel(cfg)
    m.init_params(1)
    out = []
    for shape in args.shapes.split(','):
        G, K, Q = SHAPES[shape]
        rng = np.random.RandomState(G * K)
        support = rng.randint(0, cfg['input_size'], size=(G * K, T)).astype(np.int32)
        query = rng.randint(0, cfg['input_size'], size=(G * Q, T)).astype(np.int32)
        group = np.repeat(np.arange(G), Q).astype(np.int32)
        R = G * Q
        cache = m.cache_build(support, n_groups=G)
        tc, ts, tb = alternating_medians([lambda: m.cache_score(cache, query, thetas, [0.25], group=group),
                                          lambda: m.score(query),
                                          lambda: m.cache_build(support, n_groups=G).close()], args.reps)
        # the kernel's own time: event timers force eager launches, so this is a run of its own
        m.timing_select('cache_attend')
        m.timing_enable(True)
        m.timing_reset()
        for _ in range(3):
            m.cache_score(cache, query, thetas, [0.25], group=group)
        ms, launches = m.timing_read('cache_attend')
        m.timing_enable(False)
        m.timing_select(None)
        kernel_s = ms * 1e-3 / 3
        flop = 2.0 * R * T * K * T * cfg['hidden_size']
        r = dict(config=args.config, shape=shape, groups=G, support_per_group=K, query_rows=R, max_len=T, entries_per_group=K * T,
                 n_theta=len(thetas), cache_score_seconds=tc, cache_score_us_per_song=1e6 * tc / R, score_seconds=ts,
                 score_us_per_song=1e6 * ts / R, cache_score_over_score=tc / ts, cache_build_seconds=tb,
                 cache_build_us_per_song=1e6 * tb / (G * K), attend_kernel_seconds=kernel_s, attend_launches_per_call=launches / 3,
                 attend_tflops=flop / kernel_s / 1e12, attend_fraction_of_f32_mfma_peak=flop / kernel_s / PEAK_F32_MFMA,
                 attend_fraction_of_f64_mfma_peak=flop / kernel_s / PEAK_F64_MFMA, attend_over_rest_of_call=kernel_s / max(tc - kernel_s, 1e-12))
        out.append(r)
        print('%s %-7s (%d x %d support, %d query rows, T %d): cache_score %8.1f us/song | score %8.1f us/song | %.2fx | build %8.1f us/song | '
              'attention %.3f ms per call, %.2f TFLOP/s = %.1f %% of the fp32 MFMA peak (%.1f %% of fp64)'
              % (args.config, shape, G, K, R, T, r['cache_score_us_per_song'], r['score_us_per_song'], r['cache_score_over_score'],
                 r['cache_build_us_per_song'], 1e3 * kernel_s, r['attend_tflops'], 100 * r['attend_fraction_of_f32_mfma_peak'],
                 100 * r['attend_fraction_of_f64_mfma_peak']))
        cache.close()
    m.close()
    for r in out:
        print(json.dumps(r))
    if args.json:
        with open(args.json, 'w') as f:
            for r in out:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
