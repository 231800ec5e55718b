#!/usr/bin/env python3
"""Wall time per song of fsmg_score -- with every output, and with the row NLL only -- against fsmg_eval_batch on the same rows and
the same handle, at cfg-B and cfg-C dims with max_len 128, the three calls alternating within each repetition.  Prints one line
per case and one JSON line per case (--json FILE also writes them to a file).

  python tools/score_bench.py [--reps 7] [--configs cfg-B,cfg-C] [--rows 128,320] [--pass-rows 64,128,320] [--json FILE]

us/song = wall time of one call (median of --reps after one warm-up call of each) / rows.  Every call ends in its device-to-host
copy, so the wall time covers the device work.  fsmg_eval_batch reads the rows as one episode of `rows` query songs; it never
writes the [rows * max_len, V1p] logits that fsmg_score writes and reads back, so the ratio is the price of the per-token outputs."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='cfg-B,cfg-C')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--rows', default='128,320')
    ap.add_argument('--pass-rows', default='64,128,320')
    ap.add_argument('--max-len', type=int, default=128)
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    from fsmg.binding import FsmgModel
    out = []
    T = args.max_len
    for name in args.configs.split(','):
        cfg = dict(CONFIGS[name], name='lstm_baseline', seed=1, max_len=T, lr=1e-3, max_grad_norm=5, n_decay=1000)
        m = FsmgModel(cfg)
        m.init_params(1)
        for R in [int(x) for x in args.rows.split(',')]:
            songs = np.random.RandomState(R).randint(0, cfg['input_size'], size=(R, T)).astype(np.int32)
            episode = songs.reshape(1, 1, R, T)
            for P in [int(x) for x in args.pass_rows.split(',')]:
                ta, tn, te = alternating_medians(
                    [lambda: m.score(songs, logprob=True, rank=True, entropy=True, argmax=True, row_nll=True, pass_rows=P),
                     lambda: m.score(songs, logprob=False, row_nll=True, pass_rows=P),
                     lambda: m.eval_batch(episode)], args.reps)
                r = dict(config=name, rows=R, max_len=T, pass_rows=P, score_all_seconds=ta, score_all_us_per_song=1e6 * ta / R,
                         score_nll_seconds=tn, score_nll_us_per_song=1e6 * tn / R, eval_seconds=te, eval_us_per_song=1e6 * te / R,
                         score_all_over_eval=ta / te, score_nll_over_eval=tn / te)
                out.append(r)
                print('%s rows=%-3d pass_rows=%-3d: score(all) %8.1f us/song | score(row_nll) %8.1f us/song | eval_batch %8.1f us/song | '
                      '%.2fx %.2fx' % (name, R, P, r['score_all_us_per_song'], r['score_nll_us_per_song'], r['eval_us_per_song'],
                                       r['score_all_over_eval'], r['score_nll_over_eval']))
        m.close()
    for r in out:
        print(json.dumps(r))
    if args.json:
        with open(args.json, 'w') as f:
            for r in out:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
