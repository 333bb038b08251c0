"""configs[2] beamed decode (depth 4, width 512, V 256, N = 8, 1024 x 100 characters, the bench's weights): ms per call of the
default search and of the search with "lm_predict" (children rated by the decoder's context-free LM), 1 warm-up call then 3 timed
ones per setting on one handle, wall clock around HipEngine.decode_beam (encoder included), then one call per setting with the
library's per-kernel HIP-event timing (casv_profile level 1: its events cost some of the time) for the kernel split.

    python3 profiles/c3_lm_predict_timing.py [default|lm_predict] [--out FILE.json]

With one of the two names only that setting runs (for a rocprofv3 --kernel-trace --stats run of one of them); --out writes every
call's time and the kernel split as JSON (profiles/r07_c3_lm_predict_timing.json)."""
import json
import os
import sys
import time

import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ModelConfig, make_weights, make_lines
from cor_asv_ann_amd.engine import HipEngine
DEPTH, WIDTH, VOC, LINES, LENGTH, BEAM_N, LINE_SEED, EMB_SCALE = 4, 512, 256, 1024, 100, 8, 103, 128.0   # bench.py configs[2]
cfg = ModelConfig(depth=DEPTH, width=WIDTH, voc_size=VOC)
w = make_weights(cfg, emb_scale=EMB_SCALE)
_, idx = make_lines(LINES, LENGTH, LINE_SEED, voc_size=VOC)
args = sys.argv[1:]
out_file = None
if '--out' in args:
    k = args.index('--out'); out_file = args[k + 1]; del args[k:k + 2]
only = args[0] if args else None
CLASSES = ('lstm_gemm', 'lstm_gemm_small', 'gemm', 'attention', 'softmax', 'beam', 'embed', 'persist')
eng = HipEngine(DEPTH, WIDTH, VOC)
eng.set_weights(w)
out = {}
for name, lm in (('default', 0), ('lm_predict', 1)):
    if only and name != only:
        continue
    eng.set_option('lm_predict', lm)
    eng.encode(idx)
    res = eng.decode_beam(batch_size=BEAM_N)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter(); eng.encode(idx); res = eng.decode_beam(batch_size=BEAM_N); ts.append((time.perf_counter() - t0) * 1e3)
    steps = int(res['n_steps'].max())
    eng.profile(True)
    eng.encode(idx); eng.decode_beam(batch_size=BEAM_N)
    split = {}
    for c in CLASSES:
        r = eng.profile_read(c)
        if r['launches']:
            split[c] = {'launches': int(r['launches']), 'ms': round(float(r['ms']), 3)}
    eng.profile(False)
    out[name] = {'median_ms': float(np.median(ts)), 'min_ms': float(np.min(ts)), 'calls_ms': ts, 'search_iterations': steps,
                 'kernels_profiled_call': split}
eng.close()
print(json.dumps({k: (v['median_ms'], v['min_ms']) for k, v in out.items()}))
if out_file:
    with open(out_file, 'w') as f:
        json.dump(out, f, indent=1)
