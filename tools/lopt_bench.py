#!/usr/bin/env python3
"""What the learned optimiser (a meta-learner LSTM cell per parameter element) costs in the MAML-style step at cfg-E
(5-way, 5 support + 4 query songs, max_len 50, 2 x 1024 hidden, one inner step), the legs alternating in one warmed process, and its
event-timed kernels beside k_sgd_update.  Prints one line per leg and kernel and one JSON line; --out PREFIX writes PREFIX.txt and
PREFIX.json (profiles/lopt_bench.*).

  python tools/lopt_bench.py [--reps 5] [--steps 20] [--out profiles/lopt_bench]

A leg is --steps fsmg_maml_step calls on one handle without a read-back and a synchronising read at the end; ms/step = wall time /
steps, the median over --reps.  Legs:
  disabled_a, disabled_b   a handle that never enabled the learned optimiser, twice: their ratio is the yardstick (A/A)
  enabled                  a second handle, enabled with a non-trivial Phi and phi_lr > 0: per step two fills (F, I), one
                           k_lopt_update<store> in place of k_sgd_update, k_lopt_backprop<1>, k_lopt_phi twice (the reduction, the update)
Kernels (the library's per-class event timers, eager launches): bytes/s = bytes per parameter x flat parameter count / mean time.
Bytes per parameter as the kernels are written: k_sgd_update 12, k_lopt_update 28 (eval forms) and 32 (train forms: + the stored
gradient), k_lopt_backprop (K + 3) x 4 = 16 at K = 1.  k_lopt_phi moves 2048 x 14 doubles: its time is reported without a rate.
No threshold: the numbers are reported."""
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
KERNELS = [('sgd_update', 'k_sgd_update', 12), ('lopt_update', 'k_lopt_update<false>', 28), ('lopt_update_store', 'k_lopt_update<true>', 32),
           ('lopt_backprop', 'k_lopt_backprop<1>', 4 * (INNER_STEPS + 3)), ('lopt_phi', 'k_lopt_phi (reduce)', 0), ('lopt_phi_update', 'k_lopt_phi (update)', 0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--kernel-calls', type=int, default=10)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    from fsmg.binding import FSMG_GRAD_TAIL, FsmgModel
    T, V = CFG_E['max_len'], CFG_E['input_size']
    rng = np.random.RandomState(7)
    sup = rng.randint(0, V, size=(N, K, T)).astype(np.int32)
    qry = rng.randint(0, V, size=(N, Q, T)).astype(np.int32)
    plain = FsmgModel(CFG_E, max_sequences=N * (K + Q))
    learned = FsmgModel(CFG_E, max_sequences=N * (K + Q))
    for m in (plain, learned):
        m.init_params(1)
    learned.lopt_enable(phi_lr=1e-3, max_train_steps=INNER_STEPS)
    phi = np.zeros(14, np.float32)
    phi[0:6], phi[6] = rng.uniform(-0.3, 0.3, 6), 2.0
    phi[7:13], phi[13] = rng.uniform(-0.3, 0.3, 6), 0.25
    learned.lopt_set_phi(phi)
    n_flat = plain.grad_buffer()[1] - FSMG_GRAD_TAIL

    def leg(m):
        def run():
            for _ in range(args.steps - 1):
                m.maml_step(sup, qry, INNER_STEPS, INNER_LR, want_loss=False)
            m.maml_step(sup, qry, INNER_STEPS, INNER_LR, want_loss=True)       # the read-back ends the leg: every step has retired
        return run
    legs = [('disabled_a', leg(plain)), ('enabled', leg(learned)), ('disabled_b', leg(plain))]
    for _, fn in legs:                       # warm: first calls, allocations, schedule decisions, captured graphs
        fn()
    times = {name: [] for name, _ in legs}
    for _ in range(args.reps):
        for name, fn in legs:
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    out = dict(config='cfg-E', rows_support=N * K, rows_query=N * Q, max_len=T, inner_steps=INNER_STEPS, steps=args.steps, reps=args.reps,
               n_flat=int(n_flat), timeouts=plain.stats()['timeouts'] + learned.stats()['timeouts'])
    lines = []
    for name, _ in legs:
        out[name + '_ms'] = float(np.median(times[name]))
        out[name + '_min_ms'], out[name + '_max_ms'] = float(np.min(times[name])), float(np.max(times[name]))
        lines.append('%-12s %.4f ms/step (min %.4f, max %.4f)' % (name, out[name + '_ms'], out[name + '_min_ms'], out[name + '_max_ms']))
    mean_d = 0.5 * (out['disabled_a_ms'] + out['disabled_b_ms'])
    out['aa_ratio'] = out['disabled_b_ms'] / out['disabled_a_ms']
    out['enabled_over_disabled'] = out['enabled_ms'] / mean_d
    out['enabled_minus_disabled_ms'] = out['enabled_ms'] - mean_d
    lines.append('A/A ratio %.4f | enabled / disabled %.4f (%+.4f ms)' % (out['aa_ratio'], out['enabled_over_disabled'], out['enabled_minus_disabled_ms']))

    # the kernels, event-timed one class at a time (timing runs every launch eagerly): the split train form and the eval form
    def timed(m, cls, call):
        m.timing_enable(True)
        m.timing_select(cls)
        m.timing_reset()
        for _ in range(args.kernel_calls):
            call(m)
        ms, n = m.timing_read(cls)
        m.timing_enable(False)
        m.timing_select(None)
        return ms, n

    def train_form(m):
        m.maml_forward_backward(sup, qry, INNER_STEPS, INNER_LR)
        m.apply_update(1.0, want_loss=False)
    eval_form = lambda m: m.maml_eval(sup, qry, INNER_STEPS, INNER_LR)
    runs = {'sgd_update': (plain, train_form), 'lopt_update': (learned, eval_form), 'lopt_update_store': (learned, train_form),
            'lopt_backprop': (learned, train_form), 'lopt_phi': (learned, train_form), 'lopt_phi_update': (learned, train_form)}
    out['kernels'] = {}
    for cls, kernel, bpp in KERNELS:
        ms, n = timed(*((runs[cls][0], cls, runs[cls][1])))
        us = ms / max(n, 1) * 1e3
        gbs = bpp * n_flat / (us * 1e-6) / 1e9 if us > 0 else 0.0
        out['kernels'][cls] = dict(kernel=kernel, launches=int(n), mean_us=us, bytes_per_parameter=bpp, gb_per_s=gbs)
        if bpp:
            lines.append('%-22s %8.2f us over %d launches, %7.0f GB/s against %d B x %d' % (kernel, us, n, gbs, bpp, n_flat))
        else:
            lines.append('%-22s %8.2f us over %d launches' % (kernel, us, n))
    plain.close()
    learned.close()
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
