#!/usr/bin/env python3
"""What a decode state (fsmg_dstate_*) costs, at cfg-B and cfg-C dims on one handle, the legs of each comparison
alternating within each repetition.  Prints one line per case and one JSON line per case (--json FILE also writes them to a file).

  python tools/dstate_bench.py [--num 256] [--reps 9] [--configs cfg-B,cfg-C] [--batches 1,64] [--chunks 1,4,16,64,256]
                               [--feed-rows 128] [--parts a,b,c] [--json FILE]

  a  stateful against one-shot: fsmg_dstate_generate on a fresh state (reset + generate) against fsmg_generate, num tokens; a second
     fsmg_generate leg gives the A/A noise floor |t(A') / t(A) - 1| of the same repetitions.
  b  chunk size: num tokens as 1, 4, ... calls on a fresh state; per-call overhead = (t(n calls) - t(1 call)) / (n - 1).
  c  feed against score: fsmg_dstate_feed with log-probs of --feed-rows songs of max_len = 128 tokens against fsmg_score of the same
     songs (log-probs only).

Wall time of the calls (median of --reps after one warm-up of each leg).  Every call ends in its device-to-host copy, so the wall
time covers the device work; in (b) every chunk ends in one."""
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

MAX_LEN = 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='cfg-B,cfg-C')
    ap.add_argument('--num', type=int, default=256)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--batches', default='1,64')
    ap.add_argument('--chunks', default='1,4,16,64,256')
    ap.add_argument('--feed-rows', type=int, default=128)
    ap.add_argument('--parts', default='a,b,c')
    ap.add_argument('--temperature', type=float, default=1.0)
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    from fsmg.binding import FsmgModel
    rows = []
    num, T, parts = args.num, args.temperature, args.parts.split(',')
    for name in args.configs.split(','):
        cfg = dict(CONFIGS[name], name='lstm_baseline', seed=1, max_len=MAX_LEN, lr=1e-3, max_grad_norm=5, n_decay=1000)
        m = FsmgModel(cfg)
        m.init_params(1)
        for B in [int(x) for x in args.batches.split(',')]:
            st = m.new_state(B, history=64)

            def stateful(n_calls=1):
                st.reset()
                for _ in range(n_calls):
                    m.generate(B, num // n_calls, temperature=T, seed=3, state=st)

            one_shot = lambda: m.generate(B, num, temperature=T, seed=3)
            if 'a' in parts:
                ta, tb, ts = alternating_medians([one_shot, one_shot, stateful], args.reps)
                r = dict(part='a', config=name, rows=B, num=num, generate_seconds=ta, generate_again_seconds=tb, dstate_seconds=ts,
                         generate_us_per_position=1e6 * ta / num, dstate_us_per_position=1e6 * ts / num,
                         dstate_over_generate=ts / ta, noise_floor=abs(tb / ta - 1.0))
                rows.append(r)
                print('(a) %s B=%-3d: dstate %8.2f us/position | generate %8.2f us/position | %.4fx | A/A floor %.4f'
                      % (name, B, r['dstate_us_per_position'], r['generate_us_per_position'], r['dstate_over_generate'], r['noise_floor']))
            if 'b' in parts:
                counts = [int(c) for c in args.chunks.split(',') if num % int(c) == 0]
                ts = alternating_medians([lambda n=n: stateful(n) for n in counts], args.reps)
                base = ts[counts.index(1)] if 1 in counts else None
                for n, t in zip(counts, ts):
                    over = 1e6 * (t - base) / (n - 1) if base is not None and n > 1 else 0.0
                    r = dict(part='b', config=name, rows=B, num=num, calls=n, tokens_per_call=num // n, seconds=t,
                             us_per_position=1e6 * t / num, overhead_us_per_call=over)
                    rows.append(r)
                    print('(b) %s B=%-3d: %3d calls of %3d tokens %8.2f us/position | %7.1f us per extra call'
                          % (name, B, n, num // n, r['us_per_position'], over))
            st.close()
        if 'c' in parts:
            R = args.feed_rows
            songs = np.random.RandomState(5).randint(0, cfg['input_size'], size=(R, MAX_LEN)).astype(np.int32)
            st = m.new_state(R, history=64)

            def feed():
                st.reset()
                m.feed(st, songs, logprobs=True)

            tf, tsc = alternating_medians([feed, lambda: m.score(songs, row_nll=False)], args.reps)
            r = dict(part='c', config=name, rows=R, max_len=MAX_LEN, feed_seconds=tf, score_seconds=tsc, feed_us_per_song=1e6 * tf / R,
                     score_us_per_song=1e6 * tsc / R, feed_over_score=tf / tsc)
            rows.append(r)
            print('(c) %s R=%-3d: feed %8.2f us/song | score %8.2f us/song | %.2fx'
                  % (name, R, r['feed_us_per_song'], r['score_us_per_song'], r['feed_over_score']))
            st.close()
        m.close()
    for r in rows:
        print(json.dumps(r))
    if args.json:
        with open(args.json, 'w') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
