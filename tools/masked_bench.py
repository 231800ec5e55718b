#!/usr/bin/env python3
"""What the padding-masked train step costs (fsmg_train_step_masked) against fsmg_train_step at cfg-B (45 rows,
max_len 128), the legs alternating in one warmed process.  Prints one line per leg and one JSON line (--json FILE also writes it).

  python tools/masked_bench.py [--reps 7] [--steps 40] [--timing] [--json FILE]

A leg is --steps train steps on one handle without a read-back and a synchronising read at the end; ms/step = wall time / steps, the
median over --reps.  Legs:
  unmasked_a, unmasked_b   fsmg_train_step on a uniform episode, twice: their spread is the yardstick (A/A)
  masked_full              fsmg_train_step_masked on the same episode, every length max_len (the unmasked step's arithmetic)
  unmasked_zipf            fsmg_train_step on a zero-padded Zipf episode, lengths uniform in [T/4, T] (the data changes the embedding
                           gradient's cost, so the masked leg on this episode is compared with this one)
  masked_zipf              fsmg_train_step_masked on that episode with its lengths
--timing: afterwards, the per-class kernel times (fsmg_timing_*) of one unmasked and one masked step on the Zipf episode."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'few-shot-music-generation_amd', 'src'))

CFG_B = dict(name='lstm_baseline', seed=1, input_size=10000, embedding_size=250, hidden_size=512, n_layers=1, max_len=128,
             lr=5e-3, max_grad_norm=5, n_decay=10000)
N, K, Q = 5, 5, 4
CLASSES = ('gemm_zx', 'lstm_fwd', 'gemm_logits', 'ce', 'gemm_dhout', 'gemm_dw', 'lstm_bwd', 'gemm_dk', 'gemm_dx', 'embed_grad', 'update')


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
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--timing', action='store_true')
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    from fsmg.binding import FsmgModel
    T, V = CFG_B['max_len'], CFG_B['input_size']
    rng = np.random.RandomState(7)
    sup = rng.randint(0, V, size=(N, K, T)).astype(np.int32)
    qry = rng.randint(0, V, size=(N, Q, T)).astype(np.int32)
    full_s, full_q = np.full((N, K), T, np.int32), np.full((N, Q), T, np.int32)
    zs, zq, zsl, zql = zipf_episode(rng, T, V)
    m = FsmgModel(CFG_B, max_sequences=N * (K + Q))
    m.init_params(1)

    def leg(step):
        def run():
            for _ in range(args.steps - 1):
                step(False)
            step(True)                       # the read-back ends the leg: every step has retired
        return run

    legs = [
        ('unmasked_a', leg(lambda w: m.train_step(sup, qry, want_loss=w))),
        ('masked_full', leg(lambda w: m.train_step_masked(sup, qry, full_s, full_q, want_loss=w))),
        ('unmasked_b', leg(lambda w: m.train_step(sup, qry, want_loss=w))),
        ('unmasked_zipf', leg(lambda w: m.train_step(zs, zq, want_loss=w))),
        ('masked_zipf', leg(lambda w: m.train_step_masked(zs, zq, zsl, zql, want_loss=w))),
    ]
    for _, fn in legs:                       # warm: every path's first calls, allocations, schedule decisions
        fn()
    times = {name: [] for name, _ in legs}
    for _ in range(args.reps):
        for name, fn in legs:
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    out = dict(config='cfg-B', rows=N * (K + Q), max_len=T, steps=args.steps, reps=args.reps,
               n_valid_zipf=int(zsl.sum() + zql.sum()), positions=N * (K + Q) * T)
    for name, _ in legs:
        out[name + '_ms'] = float(np.median(times[name]))
        out[name + '_min_ms'], out[name + '_max_ms'] = float(np.min(times[name])), float(np.max(times[name]))
        print('%-14s %.4f ms/step (min %.4f, max %.4f)' % (name, out[name + '_ms'], out[name + '_min_ms'], out[name + '_max_ms']))
    out['aa_spread_ms'] = abs(out['unmasked_a_ms'] - out['unmasked_b_ms'])
    out['masked_full_minus_unmasked_ms'] = out['masked_full_ms'] - 0.5 * (out['unmasked_a_ms'] + out['unmasked_b_ms'])
    out['masked_zipf_minus_unmasked_zipf_ms'] = out['masked_zipf_ms'] - out['unmasked_zipf_ms']
    print('A/A spread %.4f ms | masked(full) - unmasked %+.4f ms | masked(zipf) - unmasked(zipf) %+.4f ms'
          % (out['aa_spread_ms'], out['masked_full_minus_unmasked_ms'], out['masked_zipf_minus_unmasked_zipf_ms']))
    if args.timing:
        for tag, step in (('unmasked_zipf', lambda: m.train_step(zs, zq)), ('masked_zipf', lambda: m.train_step_masked(zs, zq, zsl, zql))):
            m.timing_enable(True)
            m.timing_reset()
            for _ in range(5):
                step()
            per = {}
            for c in CLASSES:
                ms, n = m.timing_read(c)
                if n:
                    per[c] = ms / 5
            m.timing_enable(False)
            out['classes_' + tag + '_ms'] = per
            print(tag, ' '.join('%s %.4f' % kv for kv in sorted(per.items())))
    m.close()
    print(json.dumps(out))
    if args.json:
        with open(args.json, 'w') as f:
            f.write(json.dumps(out) + '\n')


if __name__ == '__main__':
    main()
