#!/usr/bin/env python3
"""Wall time per song of fsmg_cache_score_masked (ragged cache built with lengths) against fsmg_cache_score (uniform cache) on the
same zero-padded rows and the same handle, the calls alternating within each repetition, and the attention kernel's own time in
both (the handle's event timers, class 'cache_attend', in runs of their own).  The unmasked call is timed TWICE per repetition: the
ratio of its two medians is the run-to-run noise that any masked / unmasked ratio has to be read against.  Two shapes at cfg-B dims:

  episode   5 groups x 5 support songs, 5 query songs per group (one few-shot episode)
  large     1 group of 200 support songs (25 600 slots at T 128), 640 query rows

  python tools/cachelen_bench.py [--reps 7] [--config cfg-B] [--max-len 128] [--lengths ragged|full] [--pass-rows 0] [--json FILE]

--lengths ragged: every song's length uniform in [T/4, T], the rows zero behind it (what the loader pads with); full: all T (the
masked calls must then cost what the unmasked ones do).  us/song = wall time of one call (median of --reps after one warm-up call
of each) / rows; every call ends in its device-to-host copy.  The expected saving in attention work is the kept share of the
queries times the kept share of the entries; the tool prints that product beside what it measured."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'few-shot-music-generation_amd', 'src'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from beam_bench import CONFIGS     # noqa: E402

SHAPES = {'episode': (5, 5, 5), 'large': (1, 200, 640)}          # groups, support songs per group, query songs per group


def alternating_samples(fns, reps):
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            ts[i].append(time.perf_counter() - t0)
    return [np.asarray(t) for t in ts]


def padded(rng, rows, T, vocab, lengths):
    a = rng.randint(1, vocab, size=(rows, T)).astype(np.int32)
    a[np.arange(T)[None, :] >= lengths[:, None]] = 0
    return a


def kernel_ms(m, fn, calls=3):
    m.timing_select('cache_attend')
    m.timing_enable(True)
    m.timing_reset()
    for _ in range(calls):
        fn()
    ms, launches = m.timing_read('cache_attend')
    m.timing_enable(False)
    m.timing_select(None)
    return ms / calls, launches / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='cfg-B')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--max-len', type=int, default=128)
    ap.add_argument('--shapes', default='episode,large')
    ap.add_argument('--lengths', default='ragged', choices=('ragged', 'full'))
    ap.add_argument('--theta', type=float, default=1.0)
    ap.add_argument('--pass-rows', type=int, default=0, help='rows per device pass of both calls (0 = the default, 128)')
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
        lo = max(1, T // 4)
        sl = rng.randint(lo, T + 1, size=G * K).astype(np.int32) if args.lengths == 'ragged' else np.full(G * K, T, np.int32)
        ql = rng.randint(lo, T + 1, size=G * Q).astype(np.int32) if args.lengths == 'ragged' else np.full(G * Q, T, np.int32)
        support, query = padded(rng, G * K, T, cfg['input_size'], sl), padded(rng, G * Q, T, cfg['input_size'], ql)
        group = np.repeat(np.arange(G), Q).astype(np.int32)
        R = G * Q
        uniform = m.cache_build(support, n_groups=G)
        ragged = m.cache_build(support, n_groups=G, lengths=sl)
        masked = lambda: m.cache_score(ragged, query, [args.theta], [0.25], group=group, lengths=ql, pass_rows=args.pass_rows)
        plain = lambda: m.cache_score(uniform, query, [args.theta], [0.25], group=group, pass_rows=args.pass_rows)
        tm, tp, tp2, tbm, tbp = alternating_samples([masked, plain, plain,
                                                     lambda: m.cache_build(support, n_groups=G, lengths=sl).close(),
                                                     lambda: m.cache_build(support, n_groups=G).close()], args.reps)
        km, lm = kernel_ms(m, masked)
        kp, lpn = kernel_ms(m, plain)
        kp2, _ = kernel_ms(m, plain)
        med = lambda t: float(np.median(t))
        kept_q, kept_e = float(ql.sum()) / (R * T), float(sl.sum()) / (G * K * T)
        r = dict(config=args.config, shape=shape, lengths=args.lengths, pass_rows=args.pass_rows, groups=G, support_per_group=K, query_rows=R, max_len=T,
                 slots_per_group=K * T, kept_share_of_queries=kept_q, kept_share_of_entries=kept_e, expected_attention_work=kept_q * kept_e,
                 masked_seconds=med(tm), masked_min_max=[float(tm.min()), float(tm.max())],
                 unmasked_seconds=med(tp), unmasked_min_max=[float(tp.min()), float(tp.max())],
                 unmasked_again_seconds=med(tp2), noise_unmasked_again_over_unmasked=med(tp2) / med(tp),
                 masked_over_unmasked=med(tm) / med(tp), masked_us_per_song=1e6 * med(tm) / R, unmasked_us_per_song=1e6 * med(tp) / R,
                 build_masked_seconds=med(tbm), build_unmasked_seconds=med(tbp), build_masked_over_unmasked=med(tbm) / med(tbp),
                 attend_kernel_ms_masked=km, attend_kernel_ms_unmasked=kp, attend_kernel_ms_unmasked_again=kp2,
                 attend_kernel_masked_over_unmasked=km / kp, attend_kernel_noise=kp2 / kp,
                 attend_launches_per_call_masked=lm, attend_launches_per_call_unmasked=lpn)
        out.append(r)
        print('%s %-7s %-6s (%d x %d support, %d query rows, T %d; kept %.2f of the queries, %.2f of the entries, product %.2f): '
              'cache_score masked %8.1f us/song | unmasked %8.1f us/song | %.3fx (A/A noise %.3fx) | build %.3fx | attention kernel '
              '%.3f ms masked, %.3f ms unmasked, %.3fx (A/A noise %.3fx)'
              % (args.config, shape, args.lengths, G, K, R, T, kept_q, kept_e, kept_q * kept_e, r['masked_us_per_song'],
                 r['unmasked_us_per_song'], r['masked_over_unmasked'], r['noise_unmasked_again_over_unmasked'],
                 r['build_masked_over_unmasked'], km, kp, km / kp, kp2 / kp))
        uniform.close()
        ragged.close()
    m.close()
    for r in out:
        print(json.dumps(r))
    if args.json:
        with open(args.json, 'w') as f:
            for r in out:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
