#!/usr/bin/env python3
"""What a batched pass from a carried state (fsmg_*_state) costs, the legs of each comparison alternating in one process.
Prints one line per case and one JSON line per case (--json FILE also writes them to a file).

  python tools/state_bench.py [--reps 9] [--configs cfg-B,cfg-C] [--rows 128] [--parts a,b,c] [--json FILE]

  a  fsmg_score_state (reset + one pass) against fsmg_dstate_feed with log-probs (reset + feed) and against fsmg_score, --rows songs of
     max_len = 128 tokens -- the setting of DESIGN.md 16 (c); a second fsmg_score leg gives the A/A ratio of the same repetitions.
     ASSERTED: score_state advances xcd_launches / persistent_launches / step_launches exactly as fsmg_score does -- step_launches not
     at all where fsmg_score runs a persistent kernel (cfg-B); at cfg-C dims no persistent kernel takes 128 rows, and both take
     n_layers * max_len per-step launches.
  b  fsmg_train_step_state (reset + step) against fsmg_train_step_masked, 45 rows of 128 tokens at cfg-B dims, on a handle in the serial
     order for both legs (run with FSMG_XCD_OVERLAP=0); a second masked leg gives the A/A ratio.
  c  per recurrence family: HIP-event times of the import and the export launches of a state pass (fsmg_timing classes "state_import" /
     "state_export", per pass: one import per layer, one export per layer plus the ring's), and the wall time of score_state against
     score at the family's shape -- what the import, the state token prep, the weights and the export add together.

Wall time of the calls (median of --reps after one warm-up of each leg); every call ends in a device-to-host copy."""
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
# (name, config overrides, rows, environment): one shape per recurrence family that imports a state
FAMILIES = [
    ('per-step', dict(hidden_size=512), 45, dict(FSMG_PERSISTENT='0')),
    ('column-split', dict(hidden_size=512), 45, dict(FSMG_XCD='0')),
    ('slice', dict(hidden_size=200), 45, {}),
    ('xcd-fp32', dict(hidden_size=512), 45, dict(FSMG_XCD_BX3='0')),
    ('xcd-bf16', dict(hidden_size=512), 100, {}),
    ('pair-fp32', dict(hidden_size=1024), 20, {}),
    ('pair-bf16', dict(hidden_size=1024), 45, {}),
]


def launches(m):
    s = m.stats()
    return s['xcd_launches'], s['persistent_launches'], s['step_launches']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='cfg-B,cfg-C')
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--rows', type=int, default=128)
    ap.add_argument('--parts', default='a,b,c')
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    from fsmg.binding import FsmgModel
    out, parts = [], args.parts.split(',')
    base = dict(name='lstm_baseline', seed=1, max_len=MAX_LEN, lr=1e-3, max_grad_norm=5, n_decay=1000)
    if 'a' in parts:
        for name in args.configs.split(','):
            cfg = dict(CONFIGS[name], **base)
            m = FsmgModel(cfg)
            m.init_params(1)
            R = args.rows
            songs = np.random.RandomState(5).randint(0, cfg['input_size'], size=(R, MAX_LEN)).astype(np.int32)
            st = m.new_state(R, history=64)

            def feed():
                st.reset()
                m.feed(st, songs, logprobs=True)

            def score_state():
                st.reset()
                m.score_state(st, songs)

            score = lambda: m.score(songs, row_nll=False)
            score(); score_state()
            l0 = launches(m); score(); l1 = launches(m); score_state(); l2 = launches(m)
            d_score, d_state = [b - a for a, b in zip(l0, l1)], [b - a for a, b in zip(l1, l2)]
            # the same recurrent launches as fsmg_score, counter by counter: per-step launches only where fsmg_score itself takes them
            # (no persistent kernel takes 128 rows at hidden 1024), never one per position of its own
            assert d_state == d_score and sum(d_state) > 0, (d_score, d_state)
            assert d_state[2] == 0 or d_score[2] == d_state[2] == cfg['n_layers'] * MAX_LEN, (d_score, d_state)
            ts, tss, tf, ts2 = alternating_medians([score, score_state, feed, score], args.reps)
            r = dict(part='a', config=name, rows=R, max_len=MAX_LEN, score_us_per_song=1e6 * ts / R, score_state_us_per_song=1e6 * tss / R,
                     feed_us_per_song=1e6 * tf / R, score_state_over_score=tss / ts, feed_over_score_state=tf / tss, aa_ratio=ts2 / ts,
                     launches_score=d_score, launches_score_state=d_state)
            out.append(r)
            print('(a) %s R=%d: score_state %8.2f us/song | feed %8.2f | score %8.2f | state/score %.3fx | feed/state %.2fx | A/A %.4f | launches %r'
                  % (name, R, r['score_state_us_per_song'], r['feed_us_per_song'], r['score_us_per_song'], r['score_state_over_score'],
                     r['feed_over_score_state'], r['aa_ratio'], d_state))
            st.close()
            m.close()
    if 'b' in parts:
        cfg = dict(CONFIGS['cfg-B'], **base)
        m = FsmgModel(cfg, max_sequences=45)
        m.init_params(1)
        rng = np.random.RandomState(6)
        songs = rng.randint(0, cfg['input_size'], size=(45, MAX_LEN)).astype(np.int32)
        ln = rng.randint(MAX_LEN // 2, MAX_LEN + 1, size=45).astype(np.int32)
        st = m.new_state(45, history=1)
        sup, qry = songs[:25].reshape(5, 5, MAX_LEN), songs[25:].reshape(5, 4, MAX_LEN)
        sl, ql = ln[:25].reshape(5, 5), ln[25:].reshape(5, 4)

        def state_step():
            st.reset()
            m.train_step_state(st, songs, ln)

        masked = lambda: m.train_step_masked(sup, qry, sl, ql)
        tm, tst, tm2 = alternating_medians([masked, state_step, masked], max(args.reps, 15))
        r = dict(part='b', config='cfg-B', rows=45, max_len=MAX_LEN, order_env=os.environ.get('FSMG_XCD_OVERLAP', ''),
                 masked_ms=1e3 * tm, state_ms=1e3 * tst, state_over_masked=tst / tm, aa_ratio=tm2 / tm)
        out.append(r)
        print('(b) cfg-B 45 rows: train_step_state %.3f ms | train_step_masked %.3f ms | %.4fx | A/A %.4f | FSMG_XCD_OVERLAP=%s'
              % (r['state_ms'], r['masked_ms'], r['state_over_masked'], r['aa_ratio'], r['order_env'] or 'unset'))
        st.close()
        m.close()
    if 'c' in parts:
        for fam, over, R, env in FAMILIES:
            old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            cfg = dict(CONFIGS['cfg-B'], **dict(base, **over))
            m = FsmgModel(cfg, max_sequences=R)
            for k, v in old.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
            m.init_params(1)
            songs = np.random.RandomState(7).randint(0, cfg['input_size'], size=(R, MAX_LEN)).astype(np.int32)
            st = m.new_state(R, history=1)

            def score_state():
                st.reset()
                m.score_state(st, songs)

            score = lambda: m.score(songs, row_nll=False, pass_rows=R)
            ts, tss = alternating_medians([score, score_state], args.reps)
            # HIP-event times of the import (one launch per layer) and the export (one launch per layer + the ring's)
            m.timing_enable(True)
            m.timing_reset()
            for _ in range(args.reps):
                score_state()
            (imp_ms, imp_n), (exp_ms, exp_n) = m.timing_read('state_import'), m.timing_read('state_export')
            m.timing_enable(False)
            imports = m.debug_read('state_imports', 4).tolist()
            r = dict(part='c', family=fam, rows=R, hidden=cfg['hidden_size'], score_us=1e6 * ts, score_state_us=1e6 * tss,
                     added_us=1e6 * (tss - ts), import_event_us=1e3 * imp_ms / max(imp_n, 1), export_event_us=1e3 * exp_ms / max(exp_n, 1),
                     imports=imports)
            out.append(r)
            print('(c) %-12s R=%-3d H=%-4d: import %6.1f us | export %6.1f us (events, per pass) | score %9.1f us | score_state %9.1f us (wall) | imports %r'
                  % (fam, R, cfg['hidden_size'], r['import_event_us'], r['export_event_us'], r['score_us'], r['score_state_us'], imports))
            st.close()
            m.close()
    for r in out:
        print(json.dumps(r))
    if args.json:
        with open(args.json, 'w') as f:
            for r in out:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
