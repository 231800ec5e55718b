#!/usr/bin/env python3
"""Wall time per song of fsmg_cache_self_score (pure self-cache, and the union with a support cache) against fsmg_cache_score and
fsmg_score on the same rows and the same handle, the calls alternating within each repetition, and the causal kernel's own time
(the handle's event timers, class 'cache_attend_self', in a run of their own) next to k_cache_attend's ('cache_attend').  cfg-B dims:

  episode   5 groups x 5 support songs, 5 query songs per group (one few-shot episode)
  large     1 group of 200 support songs, 640 query rows

  python tools/selfcache_bench.py [--reps 7] [--config cfg-B] [--max-len 128] [--windows 16,128] [--json FILE]

us/song = wall time of one call (median of --reps after one warm-up call of each) / rows; every call ends in its device-to-host
copy.  The own part of a call walks about T * min(T, W) / 2 (position, key) pairs per row (the key tiles no position of a query tile
sees are not walked); `own_pairs_walked` is the exact count of 32 x 16 tiles x 512, `own_pairs_full` = T * T what a full walk would
cost.  `self_kernel_row_major_ms` is the same kernel on a [row][t][H] array of as many vectors (keys Hp floats apart instead of
rows * Hp).

The generation leg: us per generated position (wall time of one call of --num tokens / num; all rows together) of
fsmg_cache_self_generate (own history alone, and the union) against fsmg_cache_generate and fsmg_generate at the same rows, seed and
temperature, alternating, and the three decode-time kernels' own times per position (classes 'self_file', 'self_scores',
'cache_mix_self') next to the support path's ('cache_scores', 'cache_mix')."""
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

SHAPES = {'episode': (5, 5, 5), 'large': (1, 200, 640)}          # groups, support songs per group, query songs per group


def own_tiles(T, W):
    """16-key tiles the causal kernel walks for one row's own keys"""
    n = 0
    for t0 in range(0, T, 32):
        lo, hi = max(0, t0 - W), min(t0 + 31, T - 1)
        n += (hi - lo + 15) // 16 if hi > lo else 0
    return n


def kernel_ms(m, name, fn, calls=3):
    m.timing_select(name)
    m.timing_enable(True)
    m.timing_reset()
    for _ in range(calls):
        fn()
    ms, launches = m.timing_read(name)
    m.timing_enable(False)
    m.timing_select(None)
    return ms / calls, launches / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='cfg-B')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--max-len', type=int, default=128)
    ap.add_argument('--shapes', default='episode,large')
    ap.add_argument('--windows', default='16,128')
    ap.add_argument('--num', type=int, default=96)
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    from fsmg.binding import FsmgModel
    T = args.max_len
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
        vecs = (rng.normal(size=(R, T, cfg['hidden_size'])) * 0.1).astype(np.float32)
        for W in [int(w) for w in args.windows.split(',')]:
            pure = lambda: m.cache_self_score(query, [1.0], [0.25], W)
            union = lambda: m.cache_self_score(query, [1.0], [0.25], W, cache=cache, group=group)
            sup = lambda: m.cache_score(cache, query, [1.0], [0.25], group=group)
            tp, tu, tc, ts = alternating_medians([pure, union, sup, lambda: m.score(query)], args.reps)
            kp, _ = kernel_ms(m, 'cache_attend_self', pure)
            ku, _ = kernel_ms(m, 'cache_attend_self', union)
            kc, _ = kernel_ms(m, 'cache_attend', sup)
            # the same kernel on a row-major [row][t][H] copy of as many vectors (the raw entry point): what filing a copy of the
            # pass's time-major states first would buy the key walk
            kr, _ = kernel_ms(m, 'cache_attend_self', lambda: m.cache_self_attend(vecs, query, [1.0], W))
            r = dict(config=args.config, shape=shape, groups=G, support_per_group=K, query_rows=R, max_len=T, window=W,
                     entries_per_group=K * T, self_score_us_per_song=1e6 * tp / R, union_score_us_per_song=1e6 * tu / R,
                     cache_score_us_per_song=1e6 * tc / R, score_us_per_song=1e6 * ts / R, self_over_score=tp / ts,
                     union_over_cache_score=tu / tc, self_kernel_ms=kp, self_kernel_row_major_ms=kr, union_kernel_ms=ku, support_kernel_ms=kc,
                     own_pairs_walked=own_tiles(T, W) * 512, own_pairs_full=T * T)
            out.append(r)
            print('%s %-7s W %4d (%d x %d support, %d query rows, T %d): self %8.1f | union %8.1f | cache_score %8.1f | score %8.1f us/song | '
                  'kernels: self %.3f ms (row-major copy %.3f ms), union %.3f ms, support alone %.3f ms | own pairs walked %d of %d'
                  % (args.config, shape, W, G, K, R, T, r['self_score_us_per_song'], r['union_score_us_per_song'],
                     r['cache_score_us_per_song'], r['score_us_per_song'], kp, kr, ku, kc, r['own_pairs_walked'], r['own_pairs_full']))
        if shape == 'episode':         # 25 rows over 5 x 640 entries: one episode's artists continued
            num = args.num
            for W in [int(w) for w in args.windows.split(',')]:
                g = dict(temperature=1.0, seed=3)
                own = lambda: m.cache_self_generate(R, num, 1.0, 0.25, W, **g)
                union = lambda: m.cache_self_generate(R, num, 1.0, 0.25, W, cache=cache, group=group, **g)
                sup = lambda: m.cache_generate(cache, R, num, 1.0, 0.25, group=group, **g)
                to, tu, tc, tg = alternating_medians([own, union, sup, lambda: m.generate(R, num, **g)], args.reps)
                k = {}
                for name, fn in (('self_file', own), ('self_scores', own), ('cache_mix_self', own), ('cache_mix_self_union', union),
                                 ('cache_scores', sup), ('cache_mix', sup)):
                    k[name] = kernel_ms(m, name.replace('_union', ''), fn)[0] / num
                r = dict(config=args.config, shape=shape + '-generate', rows=R, num=num, window=W, entries_per_group=K * T,
                         self_generate_us_per_position=1e6 * to / num, union_generate_us_per_position=1e6 * tu / num,
                         cache_generate_us_per_position=1e6 * tc / num, generate_us_per_position=1e6 * tg / num,
                         kernel_ms_per_position=k)
                out.append(r)
                print('%s generate W %4d (%d rows, %d tokens): self %7.1f | union %7.1f | cache_generate %7.1f | generate %7.1f us/position | '
                      'kernels per position: file %.4f ms, own scores %.4f ms, mix (own) %.4f ms, mix (union) %.4f ms; support scores %.4f ms, mix %.4f ms'
                      % (args.config, W, R, num, r['self_generate_us_per_position'], r['union_generate_us_per_position'],
                         r['cache_generate_us_per_position'], r['generate_us_per_position'], k['self_file'], k['self_scores'],
                         k['cache_mix_self'], k['cache_mix_self_union'], k['cache_scores'], k['cache_mix']))
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
