#!/usr/bin/env python3
"""What dynamic evaluation costs (fsmg_dyneval_eval_step) at cfg-B dims (5-way, 5 support + 4 query songs, max_len 128,
hidden 512), the legs alternating in one warmed process, and what its fused update kernel reaches.  Prints one line per leg and one
JSON line; --out PREFIX also writes PREFIX.txt and PREFIX.json (profiles/dyneval_bench).

  python tools/dyneval_bench.py [--reps 5] [--out profiles/dyneval_bench]

A leg is one call on one episode, ended by its own read-back; ms/episode = wall time, the median over --reps.  Legs:
  eval_masked_a, eval_masked_b  fsmg_eval_step_masked on the query rows, twice: their ratio is the yardstick (A/A)
  maml_eval_masked              fsmg_maml_eval_masked, one inner step: one masked train pass over the support rows, one update, one forward
  dyneval_s32, dyneval_sT       fsmg_dyneval_eval_step, RMS rule, rows_per_step = K, seg_len 32 and max_len: per artist ceil(T / S) window
                                passes (forward + backward) and updates over the support block, the same over the query block
Then, with event timing on (fsmg_timing_*: eager launches), the update kernel's own time per launch ('dyneval_update') and its
bytes/s against 20 B x n_flat (theta_l read and written, theta_g, g and ms_sum read)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'few-shot-music-generation_amd', 'src'))

# bench.py's cfg-B (BASELINE.json configs[1])
CFG_B = dict(name='lstm_baseline', seed=1234, input_size=10000, max_len=128, embedding_size=250, hidden_size=512, n_layers=1, lr=5e-3,
             max_grad_norm=5, n_decay=10000)
N, K, Q = 5, 5, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    from fsmg.binding import FsmgModel
    T, V = CFG_B['max_len'], CFG_B['input_size']
    rng = np.random.RandomState(7)
    sup = rng.randint(0, V, size=(N, K, T)).astype(np.int32)
    qry = rng.randint(0, V, size=(N, Q, T)).astype(np.int32)
    sl = rng.randint(T // 4, T + 1, size=(N, K)).astype(np.int32)
    ql = rng.randint(T // 4, T + 1, size=(N, Q)).astype(np.int32)
    m = FsmgModel(CFG_B, max_sequences=N * (K + Q))
    m.init_params(1)
    for _ in range(2):                       # the statistics: two train passes at the initial parameters
        m.forward_backward_masked(sup, qry, sl, ql)
        m.dyneval_stats_accumulate()
    count, mean_rms = m.dyneval_stats_info()
    dyn = lambda S: dict(rule='rms', seg_len=S, rows_per_step=K, lr=1e-4, decay=0.02, eps=1e-3, clip_norm=5.0)
    legs = [
        ('eval_masked_a', lambda: m.eval_step_masked(qry, ql)),
        ('maml_eval_masked', lambda: m.maml_eval_masked(sup, qry, sl, ql, 1, 0.1)),
        ('dyneval_s32', lambda: m.dyneval_eval_step(dyn(32), sup, qry, sl, ql)),
        ('eval_masked_b', lambda: m.eval_step_masked(qry, ql)),
        ('dyneval_sT', lambda: m.dyneval_eval_step(dyn(T), sup, qry, sl, ql)),
    ]
    nll = {}
    for name, fn in legs:                    # warm: every path's first calls, allocations, schedule decisions
        nll[name] = float(fn())
    times = {name: [] for name, _ in legs}
    for _ in range(args.reps):
        for name, fn in legs:
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    n_flat = (m.state_bytes(CFG_B) // 4 - 16) // 4
    out = dict(config='cfg-B', N=N, K=K, Q=Q, max_len=T, reps=args.reps, stats_count=count, mean_rms=mean_rms, n_flat=int(n_flat), nll=nll)
    lines = []
    for name, _ in legs:
        out[name + '_ms'] = float(np.median(times[name]))
        out[name + '_min_ms'], out[name + '_max_ms'] = float(np.min(times[name])), float(np.max(times[name]))
        lines.append('%-18s %.3f ms/episode (min %.3f, max %.3f)  nll %.4f' % (name, out[name + '_ms'], out[name + '_min_ms'], out[name + '_max_ms'], nll[name]))
    out['aa_ratio'] = out['eval_masked_b_ms'] / out['eval_masked_a_ms']
    for S, name in ((32, 'dyneval_s32'), (T, 'dyneval_sT')):
        out[name + '_window_passes'] = int(2 * N * -(-T // S))
    # the update kernel alone: event timing replaces graph replay by the same launches issued eagerly
    m.timing_enable(True)
    m.timing_select('dyneval_update')
    m.timing_reset()
    m.dyneval_eval_step(dyn(32), sup, qry, sl, ql)
    ms, launches = m.timing_read('dyneval_update')
    m.timing_enable(False)
    out['update_launches'], out['update_us'] = int(launches), (1e3 * ms / launches if launches else float('nan'))
    out['update_bytes'] = int(20 * n_flat)
    out['update_gbps'] = out['update_bytes'] / (out['update_us'] * 1e-6) / 1e9 if launches else float('nan')
    out['timeouts'] = m.stats()['timeouts']
    lines.append('A/A ratio %.4f | update kernel %.2f us over %d launches, %.0f GB/s against 20 B x %d' %
                 (out['aa_ratio'], out['update_us'], out['update_launches'], out['update_gbps'], n_flat))
    m.close()
    for l in lines:
        print(l)
    print(json.dumps(out))
    if args.out:
        with open(args.out + '.txt', 'w') as f:
            f.write('\n'.join(lines) + '\n')
        with open(args.out + '.json', 'w') as f:
            f.write(json.dumps(out) + '\n')


if __name__ == '__main__':
    main()
