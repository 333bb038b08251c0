"""configs[3] train step (depth 4, width 512, V 256, 512 x 100 characters, dropout masks, mode 1): ms per step of the default and
the "deterministic" step, 3 warm-up steps then 10 timed ones per handle, wall clock around HipEngine.train_step.

    python3 profiles/c4_deterministic_timing.py [default|deterministic] [--out FILE.json]

With one of the two names only that step runs (for a rocprofv3 --kernel-trace --stats run of one of them); --out writes every
step's time as JSON (profiles/r07_c4_deterministic_timing.json)."""
import json
import os
import sys
import time

import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ModelConfig, make_weights
from tests.golden.make_c4_golden import DEPTH, WIDTH, VOC, c4_inputs
from cor_asv_ann_amd.engine import HipEngine
cfg = ModelConfig(depth=DEPTH, width=WIDTH, voc_size=VOC)
w = make_weights(cfg, emb_scale=4.0)
sidx, di, do, wts, masks = c4_inputs()
args = sys.argv[1:]
out_file = None
if '--out' in args:
    k = args.index('--out'); out_file = args[k + 1]; del args[k:k + 2]
only = args[0] if args else None
out = {}
for name, det in (('default', 0), ('deterministic', 1)):
    if only and name != only:
        continue
    eng = HipEngine(DEPTH, WIDTH, VOC)
    eng.set_weights(w)
    eng.set_option('deterministic', det)
    eng.train_begin()
    for _ in range(3):
        eng.train_step(sidx, None, di, do, wts, masks, mode=1)
    ts = []
    for _ in range(10):
        t0 = time.perf_counter(); eng.train_step(sidx, None, di, do, wts, masks, mode=1); ts.append((time.perf_counter() - t0) * 1e3)
    out[name] = {'median_ms': float(np.median(ts)), 'min_ms': float(np.min(ts)), 'steps_ms': ts}
    eng.train_end(); eng.close()
print(json.dumps({k: (v['median_ms'], v['min_ms']) for k, v in out.items()}))
if out_file:
    with open(out_file, 'w') as f:
        json.dump(out, f, indent=1)
