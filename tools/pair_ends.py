#!/usr/bin/env python3
"""Where the two kernel pairs of the XCD-partitioned step end, from a rocprofv3 rocpd trace of bench.py (cfg-B): per step, relative to the
step's first kernel, the end of the forward chain, of the gated projection's two work-queue launches (the forward pair's end is the later
one), of the BPTT chain and of dW's queue launches -- median, min and max over 16 consecutive steps (step_timeline.py prints ONE step).
  python tools/pair_ends.py <trace.db> [first step, default 32]"""
import sqlite3, sys
db = sqlite3.connect(sys.argv[1]); first = int(sys.argv[2]) if len(sys.argv) > 2 else 32
rows = db.execute("select name, start, end from kernels order by start").fetchall()
idx = [i for i, r in enumerate(rows) if 'k_token_prep' in r[0]]
WHAT = [('forward chain end', 'k_lstm_fwd_xcd16'), ('projection queue launches end (forward pair)', 'k_gemm_bx3h<0, 1, false, 2, true'),
        ('BPTT chain end', 'k_lstm_bwd_xcd16'), ('dW queue launches end (backward pair)', 'k_gemm_bx3h<1, 1, false, 3, true'), ('step span', '')]
acc = {w: [] for w, _ in WHAT}
for s in range(first, min(first + 16, len(idx) - 1)):
    seg = rows[idx[s]:idx[s + 1]]; t0 = seg[0][1]
    for w, pat in WHAT:
        ends = [(e - t0) / 1e3 for n, _, e in seg if pat in n]
        if ends: acc[w].append(max(ends))
for w, _ in WHAT:
    v = sorted(acc[w])
    if v: print('%-46s median %7.1f us  min %7.1f  max %7.1f  (%d steps)' % (w, v[len(v) // 2], v[0], v[-1], len(v)))
