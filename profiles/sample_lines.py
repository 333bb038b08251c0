"""What sampling costs: decode_sample on 128 sources x 8 samples against the per-step greedy decode of 1024 lines -- the same 1024
decoder rows per step, the same per-step launches apart from the pick (sample_kernel against softmax_kernel), an eighth of the
encoder.  Depth 4, width 512, V 256, lines of 100 positions, S = 200 steps, both in arithmetic 2 (the sampling entry's own), the
greedy decode with "persistent" 0 (mode 0: S steps for every line).  Also 1024 sources x 1 sample: the same encoder on both sides.

One handle, one process, alternating: per run >= 100 ms of the same call as warm-up, then the median of CALLS calls (each: encode,
decode, results on the host); RUNS runs each.  "spread" = largest minus smallest of a call's run medians.  The kernels' times per
step come from a separate profiled call each (casv_profile_read: classes "sample" and "softmax"), with top_k = 0 and 8.

    python profiles/sample_lines.py [--out FILE] [--commit ID]
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

DEPTH, WIDTH, VOC, SOURCES, SAMPLES, LENGTH = 4, 512, 256, 128, 8, 100
CALLS, RUNS = 5, 3


def median_ms(call):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.1:
        call()
    ts = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sample_lines.json'))
    ap.add_argument('--commit', default='')
    args = ap.parse_args()
    from cor_asv_ann_amd.engine import HipEngine
    from cor_asv_ann_amd.synthetic import ModelConfig, make_weights, make_lines
    cfg = ModelConfig(depth=DEPTH, width=WIDTH, voc_size=VOC)
    weights = make_weights(cfg, emb_scale=4.0)
    rows = SOURCES * SAMPLES
    _, sidx = make_lines(rows, LENGTH - 1, 104, voc_size=VOC)           # (rows, LENGTH): the characters and the end-of-line
    S = 2 * LENGTH

    eng = HipEngine(DEPTH, WIDTH, VOC)
    eng.set_weights(weights)
    eng.set_option('arithmetic', 2)
    eng.set_option('persistent', 0)

    def sample(n_sources, n, top_k=0):
        def call():
            eng.encode(sidx[:n_sources])
            return eng.decode_sample(n, top_k=top_k, seed=1)
        return call

    def greedy():
        eng.encode(sidx)
        return eng.decode_greedy(mode=0)
    calls = {'sample_%dx%d' % (SOURCES, SAMPLES): sample(SOURCES, SAMPLES), 'sample_%dx1' % rows: sample(rows, 1), 'greedy_%d' % rows: greedy}
    for call in calls.values():
        call()
    medians = {k: [] for k in calls}
    for run in range(RUNS):
        for name in (list(calls) if run % 2 == 0 else list(calls)[::-1]):
            medians[name].append(median_ms(calls[name]))

    def profiled(call):
        call()
        eng.profile(True)
        call()
        out = {c: eng.profile_read(c) for c in ('sample', 'softmax', 'lstm_gemm', 'gemm', 'attention')}
        eng.profile(False)
        return {c: {'launches': int(v['launches']), 'us_per_launch': 1e3 * v['ms'] / max(int(v['launches']), 1)} for c, v in out.items()}
    prof = {'sample_%dx%d' % (SOURCES, SAMPLES): profiled(sample(SOURCES, SAMPLES)),
            'sample_%dx%d_top_k_8' % (SOURCES, SAMPLES): profiled(sample(SOURCES, SAMPLES, 8)),
            'sample_%dx%d_top_k_64' % (SOURCES, SAMPLES): profiled(sample(SOURCES, SAMPLES, 64)),
            'sample_%dx1' % rows: profiled(sample(rows, 1)), 'greedy_%d' % rows: profiled(greedy)}
    gi, lp, lq, length, _ = sample(SOURCES, SAMPLES)()
    eng.close()
    med = {k: float(np.median(v)) for k, v in medians.items()}
    out = {'what': 'decode_sample (%d sources x %d samples, and %d x 1) against decode_greedy(mode 0, persistent 0) on %d lines: depth %d '
                   'width %d V %d, %d positions, S = %d, arithmetic 2; a call = encode + decode + results on the host; median of %d '
                   'calls per run, %d runs each, alternating, 100 ms of warm-up per run; kernel classes from one profiled call each'
                   % (SOURCES, SAMPLES, rows, rows, DEPTH, WIDTH, VOC, LENGTH, S, CALLS, RUNS),
           'host': socket.gethostname(), 'commit': args.commit,
           'run_medians_ms': medians, 'median_ms': med, 'spread_ms': {k: float(max(v) - min(v)) for k, v in medians.items()},
           'sample_over_greedy': {k: med[k] / med['greedy_%d' % rows] for k in med if k.startswith('sample')},
           'sampled_characters_per_s': float(length.sum()) / (med['sample_%dx%d' % (SOURCES, SAMPLES)] * 1e-3),
           'stepped_characters_per_s': float(rows * S) / (med['sample_%dx%d' % (SOURCES, SAMPLES)] * 1e-3),
           'profile': prof,
           'check': {'mean_length': float(length.mean()), 'mean_logp': float(np.mean([lp[b, n, :length[b, n]].mean() for b in range(SOURCES) for n in range(SAMPLES)])),
                     'distinct_lines_per_source': float(np.mean([len({gi[b, n, :length[b, n]].tobytes() for n in range(SAMPLES)}) for b in range(SOURCES)]))}}
    print(json.dumps(out))
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
