"""The search's encoder pass in the split arithmetic, per-step launches against the persistent launch (csrc/persist_split.hip):
where does the persistent form win?  The row limit of the option "persistent" = -1 (persist_plan.h, PERSIST_SPLIT_DEFAULT_ROWS) is
read off this table.

For depth 2 / width 512 / V 640 and depth 4 / width 512 / V 256, lines of 100 positions, B in {8, 40, 64, 128, 256, 512}: wall
time of casv_encode + the encoder pass + the wait for it (casv_get_encoder_outputs without output buffers: no copy) on a handle
with "arithmetic" = 2, under "persistent" = 0 and 1; per cell >= 100 ms of the same calls as warm-up, then the median of 20
calls; 3 repetitions of the whole table, forms alternating.  Input staging and the embedding are in both forms' figures alike.

    python profiles/split_persist_encoder_timing.py [--out FILE] [--commit ID]
"""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(2, 512, 640), (4, 512, 256)]
ROWS = [8, 40, 64, 128, 256, 512]
LENGTH, CALLS, REPS = 99, 20, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'split_persist_encoder_timing.json'))
    ap.add_argument('--commit', default='')
    args = ap.parse_args()
    from cor_asv_ann_amd.engine import HipEngine
    from cor_asv_ann_amd import _native as nv
    from cor_asv_ann_amd.synthetic import make_lines, make_weights
    from oracle import ModelConfig
    table = []
    for d, W, V in SHAPES:
        cfg = ModelConfig(depth=d, width=W, voc_size=V)
        eng = HipEngine(d, W, V)
        eng.set_weights(make_weights(cfg, emb_scale=64.0))
        eng.set_option('arithmetic', 2)

        def call(idx):
            eng.encode(idx)
            nv.check(eng.lib.casv_get_encoder_outputs(eng.handle, None, None))

        cells = {(B, p): [] for B in ROWS for p in (0, 1)}
        stat = {}
        for rep in range(REPS):
            for B in ROWS:
                _, idx = make_lines(B, LENGTH, 300 + B, voc_size=V)
                for p in ((0, 1) if rep % 2 == 0 else (1, 0)):
                    eng.set_option('persistent', p)
                    t0 = time.perf_counter()
                    while time.perf_counter() - t0 < 0.1:
                        call(idx)
                    stat[(B, p)] = eng.stat('encoder_persistent')
                    ts = []
                    for _ in range(CALLS):
                        t0 = time.perf_counter()
                        call(idx)
                        ts.append(time.perf_counter() - t0)
                    cells[(B, p)].append(float(np.median(ts)) * 1e3)
        for B in ROWS:
            row = {'depth': d, 'width': W, 'voc': V, 'positions': LENGTH + 1, 'rows': B,
                   'per_step_ms': cells[(B, 0)], 'persistent_ms': cells[(B, 1)],
                   'persistent_launch_ran': stat[(B, 1)], 'per_step_stat': stat[(B, 0)]}
            a, b = np.array(row['per_step_ms']), np.array(row['persistent_ms'])
            spread = max(a.max() - a.min(), b.max() - b.min())
            row['median_per_step_ms'], row['median_persistent_ms'] = float(np.median(a)), float(np.median(b))
            row['spread_ms'] = float(spread)
            row['persistent_wins'] = bool(np.median(a) - np.median(b) > spread)
            table.append(row)
            print('depth %d width %d rows %3d: per-step %s ms, persistent %s ms, spread %.3f -> %s'
                  % (d, W, B, ' '.join('%.3f' % x for x in a), ' '.join('%.3f' % x for x in b), spread,
                     'persistent wins' if row['persistent_wins'] else 'no win'), flush=True)
        eng.close()
    out = {'what': 'encoder pass of the search (arithmetic 2): casv_encode + pass + wait, median of %d calls, %d repetitions' % (CALLS, REPS),
           'commit': args.commit, 'box': socket.gethostname(), 'table': table}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
