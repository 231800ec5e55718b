#!/usr/bin/env python3
"""What dropout of the train passes costs in fsmg_train_step at cfg-B dims (5-way, 5 support + 4 query songs, max_len
128, 512 hidden, vocabulary 10 000), the legs alternating in one warmed process, and the event-timed dropout kernels beside
k_sgd_update.  Prints one line per leg and kernel and one JSON line; --out PREFIX writes PREFIX.txt and PREFIX.json
(profiles/dropout_bench.*).

  python tools/dropout_bench.py [--reps 5] [--steps 20] [--out profiles/dropout_bench]

A leg is --steps fsmg_train_step calls on one handle without a read-back and a synchronising read at the end; ms/step = wall time /
steps, the median over --reps.  Legs (one handle each, created in this order):
  default_a, default_b     a handle that never enabled dropout, twice: their ratio is the yardstick (A/A).  At cfg-B it takes the
                           XCD-partitioned order
  serial                   never enabled, created with FSMG_XCD_OVERLAP=0 FSMG_OVERLAP=0: the serial order on the kernels THAT handle picks
                           (at 45 rows the fp32 XCD-local chains)
  serial_bx3               the same with FSMG_XCD_BX3=1: the serial order on the bf16-split chains the default handle was created with --
                           the order and kernels an enabled handle runs, without the masks
  keeps_one                enabled with both keeps 1: serial_bx3's launches (bit-identical, tests/test_gpu_dropout.py)
  enabled                  enabled at keep_input 0.8 / keep_output 0.5: per step k_dropout_embed_fwd, k_dropout_fwd, two k_dropout_bwd
Kernels (the library's per-class event timers, eager launches): bytes/s = 8 B (one read, one write) x elements / mean time, the
elements being rows x padded width as the kernel walks them; k_sgd_update (12 B per parameter) is timed in the same process.
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

# bench.py's cfg-B (BASELINE.json configs[1])
CFG_B = dict(name='lstm_baseline', seed=1234, input_size=10000, max_len=128, embedding_size=250, hidden_size=512, n_layers=1, lr=5e-3,
             max_grad_norm=5, n_decay=10000)
N, K, Q = 5, 5, 4
KEEPS = dict(keep_input=0.8, keep_output=0.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--kernel-calls', type=int, default=10)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    from fsmg.binding import FsmgModel
    T, V, B = CFG_B['max_len'], CFG_B['input_size'], N * (K + Q)
    rng = np.random.RandomState(7)
    sup = rng.randint(0, V, size=(N, K, T)).astype(np.int32)
    qry = rng.randint(0, V, size=(N, Q, T)).astype(np.int32)

    def handle(env=None):
        old = {k: os.environ.get(k) for k in (env or {})}
        os.environ.update(env or {})                 # the knobs are read at fsmg_create
        try:
            m = FsmgModel(CFG_B, max_sequences=B)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        m.init_params(1)
        return m
    serial_env = dict(FSMG_XCD_OVERLAP='0', FSMG_OVERLAP='0')
    models = dict(default=handle(), serial=handle(serial_env), serial_bx3=handle(dict(serial_env, FSMG_XCD_BX3='1')), keeps_one=handle(),
                  enabled=handle())
    models['keeps_one'].dropout_enable(keep_input=1.0, keep_output=1.0, seed=3)
    models['enabled'].dropout_enable(seed=3, **KEEPS)

    def leg(m):
        def run():
            for _ in range(args.steps - 1):
                m.train_step(sup, qry, want_loss=False)
            m.train_step(sup, qry, want_loss=True)       # the read-back ends the leg: every step has retired
        return run
    legs = [('default_a', leg(models['default'])), ('serial', leg(models['serial'])), ('serial_bx3', leg(models['serial_bx3'])),
            ('keeps_one', leg(models['keeps_one'])), ('enabled', leg(models['enabled'])), ('default_b', leg(models['default']))]
    for _, fn in legs:                       # warm: first calls, allocations, schedule decisions, captured graphs
        fn()
    times = {name: [] for name, _ in legs}
    for _ in range(args.reps):
        for name, fn in legs:
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    out = dict(config='cfg-B', rows=B, max_len=T, steps=args.steps, reps=args.reps, keeps=KEEPS,
               xcd_partitioned_default=bool(models['default'].debug_read('xcd_partitioned', 3)[2]),
               timeouts=sum(m.stats()['timeouts'] for m in models.values()))
    lines = []
    for name, _ in legs:
        out[name + '_ms'] = float(np.median(times[name]))
        out[name + '_min_ms'], out[name + '_max_ms'] = float(np.min(times[name])), float(np.max(times[name]))
        lines.append('%-12s %.4f ms/step (min %.4f, max %.4f)' % (name, out[name + '_ms'], out[name + '_min_ms'], out[name + '_max_ms']))
    mean_d = 0.5 * (out['default_a_ms'] + out['default_b_ms'])
    out['aa_ratio'] = out['default_b_ms'] / out['default_a_ms']
    for name in ('serial', 'serial_bx3', 'keeps_one', 'enabled'):
        out[name + '_over_default'] = out[name + '_ms'] / mean_d
    out['enabled_over_serial_bx3'] = out['enabled_ms'] / out['serial_bx3_ms']
    out['enabled_minus_serial_bx3_ms'] = out['enabled_ms'] - out['serial_bx3_ms']
    lines.append('default takes the XCD-partitioned order: %s | A/A ratio %.4f' % (out['xcd_partitioned_default'], out['aa_ratio']))
    lines.append('over default: serial %.4f, serial_bx3 %.4f, keeps_one %.4f, enabled %.4f' % tuple(
        out[n + '_over_default'] for n in ('serial', 'serial_bx3', 'keeps_one', 'enabled')))
    lines.append('enabled / serial_bx3 %.4f (%+.4f ms): what the masks themselves cost' % (out['enabled_over_serial_bx3'], out['enabled_minus_serial_bx3_ms']))

    # the kernels, event-timed one class at a time (timing runs every launch eagerly)
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

    d = models['enabled'].debug_dims()
    rows = T * B
    n_flat = models['enabled'].msgd_info()['count']
    step = lambda m: m.train_step(sup, qry, want_loss=False)
    maml = lambda m: m.maml_forward_backward(sup, qry, 1, 0.1)
    kernels = [('dropout_embed_fwd', 'k_dropout_embed_fwd', 8, rows * d['Ep'], step), ('dropout_fwd', 'k_dropout_fwd', 8, rows * d['Hp'], step),
               ('dropout_bwd', 'k_dropout_bwd (dH)', 8, rows * d['Hp'], step), ('dropout_bwd_emb', 'k_dropout_bwd (dXemb)', 8, rows * d['Ep'], step),
               ('sgd_update', 'k_sgd_update', 12, n_flat, maml)]
    out['kernels'] = {}
    for cls, kernel, bpe, elements, call in kernels:
        ms, n = timed(models['enabled'], cls, call)
        us = ms / max(n, 1) * 1e3
        gbs = bpe * elements / (us * 1e-6) / 1e9 if us > 0 else 0.0
        out['kernels'][cls] = dict(kernel=kernel, launches=int(n), mean_us=us, bytes_per_element=bpe, elements=int(elements), gb_per_s=gbs)
        lines.append('%-24s %8.2f us over %d launches, %7.0f GB/s against %d B x %d' % (kernel, us, n, gbs, bpe, elements))
    for m in models.values():
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
