#!/usr/bin/env python3
"""What one adaptation per artist costs (fsmg_maml_tasks_step) against the joint fsmg_maml_step at cfg-E (5-way, 5 support
+ 4 query songs, max_len 50, 2 x 1024 hidden, one inner step), the legs alternating in one warmed process.  Prints one line per leg
and one JSON line (--json FILE also writes it).

  python tools/mamltask_bench.py [--reps 7] [--steps 10] [--json FILE]

A leg is --steps steps on one handle without a read-back and a synchronising read at the end; ms/step = wall time / steps, the
median over --reps.  Legs:
  joint_a, joint_b   fsmg_maml_step on the episode, twice: their ratio is the yardstick (A/A)
  tasks              fsmg_maml_tasks_step on the same episode: N adaptations of K rows, N query passes of Q rows, N folds
  twin_one           fsmg_maml_step on artist 0 alone (N = 1, rows K, Q)
  tasks_one          fsmg_maml_tasks_step on artist 0 alone: the launches of twin_one with the fold in the place of the rate-gradient /
                     restore launches -- its time should sit inside the A/A spread of twin_one_b / twin_one
  twin_one_b         twin_one again (the A/A of the one-artist legs)
Then, with event timing on (eager launches, one class at a time), the task_fold kernel's time and bytes/s beside k_sgd_update's."""
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


def kernel_time(m, cls, run):
    """total ms and launches of timing class `cls` over one `run` (event timing: eager, that class alone)"""
    m.timing_enable(True)
    m.timing_select(cls)
    m.timing_reset()
    run()
    ms, launches = m.timing_read(cls)
    m.timing_select(None)
    m.timing_enable(False)
    return ms, launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    from fsmg.binding import FsmgModel
    T, V = CFG_E['max_len'], CFG_E['input_size']
    rng = np.random.RandomState(7)
    sup = rng.randint(0, V, size=(N, K, T)).astype(np.int32)
    qry = rng.randint(0, V, size=(N, Q, T)).astype(np.int32)
    sup1, qry1 = sup[:1].copy(), qry[:1].copy()
    m = FsmgModel(CFG_E, max_sequences=N * (K + Q))
    m.init_params(1)

    def leg(step):
        def run():
            for _ in range(args.steps - 1):
                step(False)
            step(True)                       # the read-back ends the leg: every step has retired
        return run

    joint = lambda s, q: (lambda w: m.maml_step(s, q, INNER_STEPS, INNER_LR, want_loss=w))
    tasks = lambda s, q: (lambda w: m.maml_tasks_step(s, q, INNER_STEPS, INNER_LR, want_loss=w))
    legs = [
        ('joint_a', leg(joint(sup, qry))),
        ('tasks', leg(tasks(sup, qry))),
        ('joint_b', leg(joint(sup, qry))),
        ('twin_one', leg(joint(sup1, qry1))),
        ('tasks_one', leg(tasks(sup1, qry1))),
        ('twin_one_b', leg(joint(sup1, qry1))),
    ]
    for _, fn in legs:                       # warm: every path's first calls, allocations, schedule decisions, graph captures
        fn()
    times = {name: [] for name, _ in legs}
    for _ in range(args.reps):
        for name, fn in legs:
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    out = dict(config='cfg-E', artists=N, rows_support=N * K, rows_query=N * Q, max_len=T, inner_steps=INNER_STEPS, steps=args.steps,
               reps=args.reps)
    for name, _ in legs:
        out[name + '_ms'] = float(np.median(times[name]))
        out[name + '_min_ms'], out[name + '_max_ms'] = float(np.min(times[name])), float(np.max(times[name]))
        print('%-11s %.4f ms/step (min %.4f, max %.4f)' % (name, out[name + '_ms'], out[name + '_min_ms'], out[name + '_max_ms']))
    mean_j = 0.5 * (out['joint_a_ms'] + out['joint_b_ms'])
    mean_1 = 0.5 * (out['twin_one_ms'] + out['twin_one_b_ms'])
    out['aa_ratio'] = out['joint_b_ms'] / out['joint_a_ms']
    out['aa_ratio_one'] = out['twin_one_b_ms'] / out['twin_one_ms']
    out['tasks_over_joint'] = out['tasks_ms'] / mean_j
    out['tasks_one_over_twin'] = out['tasks_one_ms'] / mean_1
    # the kernels, event-timed: N folds per tasks call, N * inner_steps k_sgd_update launches beside them
    n_flat = m.grad_buffer()[1] - 16
    fold_ms, fold_n = kernel_time(m, 'task_fold', lambda: m.maml_tasks_forward_backward(sup, qry, INNER_STEPS, INNER_LR))
    sgd_ms, sgd_n = kernel_time(m, 'sgd_update', lambda: m.maml_tasks_forward_backward(sup, qry, INNER_STEPS, INNER_LR))
    m.synchronize()
    # bytes per element: the first fold moves G and P_saved in, ACC and P out (16 B), every later one ACC in as well (20 B);
    # k_sgd_update moves G and P in, P out (12 B)
    fold_bytes = 4.0 * n_flat * (4 + 5 * (fold_n - 1)) if fold_n else 0.0
    out.update(n_flat=int(n_flat), task_fold_launches=int(fold_n), task_fold_us=1e3 * fold_ms / max(fold_n, 1),
               task_fold_gbps=fold_bytes / max(fold_ms, 1e-9) / 1e6, sgd_update_launches=int(sgd_n),
               sgd_update_us=1e3 * sgd_ms / max(sgd_n, 1), sgd_update_gbps=12.0 * n_flat * sgd_n / max(sgd_ms, 1e-9) / 1e6,
               timeouts=m.stats()['timeouts'])
    print('A/A ratio %.4f | tasks / joint %.4f (N = %d) | one artist: A/A %.4f, tasks / twin %.4f'
          % (out['aa_ratio'], out['tasks_over_joint'], N, out['aa_ratio_one'], out['tasks_one_over_twin']))
    print('task_fold %.1f us, %.0f GB/s over %d launches | k_sgd_update %.1f us, %.0f GB/s over %d launches (n_flat %d)'
          % (out['task_fold_us'], out['task_fold_gbps'], fold_n, out['sgd_update_us'], out['sgd_update_gbps'], sgd_n, n_flat))
    m.close()
    print(json.dumps(out))
    if args.json:
        with open(args.json, 'w') as f:
            f.write(json.dumps(out) + '\n')


if __name__ == '__main__':
    main()
