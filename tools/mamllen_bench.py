#!/usr/bin/env python3
"""What per-song lengths cost in the MAML-style step (fsmg_maml_step_masked) against fsmg_maml_step at cfg-E (5-way,
5 support + 4 query songs, max_len 50, 2 x 1024 hidden, one inner step), the legs alternating in one warmed process.  Prints one
line per leg and one JSON line (--json FILE also writes it).

  python tools/mamllen_bench.py [--reps 7] [--steps 20] [--json FILE]

A leg is --steps steps on one handle without a read-back and a synchronising read at the end; ms/step = wall time / steps, the
median over --reps.  Legs:
  unmasked_a, unmasked_b   fsmg_maml_step on a uniform episode, twice: their ratio is the yardstick (A/A)
  masked_full              fsmg_maml_step_masked on the same episode, every length max_len (the unmasked step's arithmetic, plus
                           per pass the row-weight launch, the masked loss sum and the length copy: (inner_steps + 1) passes)
  unmasked_zipf            fsmg_maml_step on a zero-padded Zipf episode, lengths uniform in [T/4, T] (the data changes the embedding
                           gradient's cost, so the masked leg on this episode is compared with this one)
  masked_zipf              fsmg_maml_step_masked on that episode with its lengths"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'few-shot-music-generation_amd', 'src'))

# bench.py's cfg-E (BASELINE.json configs[4])
CFG_E = dict(name='maml_lstm', seed=1234, input_size=4708, max_len=50, embedding_size=250, hidden_size=1024, n_layers=2, lr=5e-3,
             max_grad_norm=5, n_decay=10000)
N, K, Q = 5, 5, 4
INNER_STEPS, INNER_LR = 1, 0.1


def zipf_episode(rng, T, vocab):
    def songs(n):
        a = np.minimum(rng.zipf(1.1, size=(N, n, T)) - 1, vocab - 1).astype(np.int32)
        lens = rng.randint(max(1, T // 4), T + 1, size=(N, n)).astype(np.int32)
        a[np.arange(T)[None, None, :] >= lens[:, :, None]] = 0
        return a, lens
    (sup, sl), (qry, ql) = songs(K), songs(Q)
    return sup, qry, sl, ql


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    from fsmg.binding import FsmgModel
    T, V = CFG_E['max_len'], CFG_E['input_size']
    rng = np.random.RandomState(7)
    sup = rng.randint(0, V, size=(N, K, T)).astype(np.int32)
    qry = rng.randint(0, V, size=(N, Q, T)).astype(np.int32)
    full_s, full_q = np.full((N, K), T, np.int32), np.full((N, Q), T, np.int32)
    zs, zq, zsl, zql = zipf_episode(rng, T, V)
    m = FsmgModel(CFG_E, max_sequences=N * (K + Q))
    m.init_params(1)

    def leg(step):
        def run():
            for _ in range(args.steps - 1):
                step(False)
            step(True)                       # the read-back ends the leg: every step has retired
        return run

    unmasked = lambda s, q: (lambda w: m.maml_step(s, q, INNER_STEPS, INNER_LR, want_loss=w))
    masked = lambda s, q, sl, ql: (lambda w: m.maml_step_masked(s, q, sl, ql, INNER_STEPS, INNER_LR, want_loss=w))
    legs = [
        ('unmasked_a', leg(unmasked(sup, qry))),
        ('masked_full', leg(masked(sup, qry, full_s, full_q))),
        ('unmasked_b', leg(unmasked(sup, qry))),
        ('unmasked_zipf', leg(unmasked(zs, zq))),
        ('masked_zipf', leg(masked(zs, zq, zsl, zql))),
    ]
    for _, fn in legs:                       # warm: every path's first calls, allocations, schedule decisions
        fn()
    times = {name: [] for name, _ in legs}
    for _ in range(args.reps):
        for name, fn in legs:
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    out = dict(config='cfg-E', rows_support=N * K, rows_query=N * Q, max_len=T, inner_steps=INNER_STEPS, steps=args.steps, reps=args.reps,
               n_valid_zipf=[int(zsl.sum()), int(zql.sum())], positions=[N * K * T, N * Q * T], timeouts=m.stats()['timeouts'])
    for name, _ in legs:
        out[name + '_ms'] = float(np.median(times[name]))
        out[name + '_min_ms'], out[name + '_max_ms'] = float(np.min(times[name])), float(np.max(times[name]))
        print('%-14s %.4f ms/step (min %.4f, max %.4f)' % (name, out[name + '_ms'], out[name + '_min_ms'], out[name + '_max_ms']))
    mean_u = 0.5 * (out['unmasked_a_ms'] + out['unmasked_b_ms'])
    out['aa_ratio'] = out['unmasked_b_ms'] / out['unmasked_a_ms']
    out['masked_full_over_unmasked'] = out['masked_full_ms'] / mean_u
    out['masked_full_minus_unmasked_ms'] = out['masked_full_ms'] - mean_u
    out['masked_zipf_over_unmasked_zipf'] = out['masked_zipf_ms'] / out['unmasked_zipf_ms']
    print('A/A ratio %.4f | masked(full) / unmasked %.4f (%+.4f ms) | masked(zipf) / unmasked(zipf) %.4f'
          % (out['aa_ratio'], out['masked_full_over_unmasked'], out['masked_full_minus_unmasked_ms'], out['masked_zipf_over_unmasked_zipf']))
    m.close()
    print(json.dumps(out))
    if args.json:
        with open(args.json, 'w') as f:
            f.write(json.dumps(out) + '\n')


if __name__ == '__main__':
    main()
