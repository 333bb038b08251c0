"""What the cut costs, and that the call without one costs what it did: profiles/sample_lines.py's shape (depth 4, width 512, V 256,
lines of 100 positions, S = 200 steps, arithmetic 2).

Per launch at R = 1024 rows, through the debug entries (casv_profile_read, class "sample"): sample_kernel at top_k 0 and 64;
sample_cut_kernel at the cuts (0, 0.9), (64, 1.0), (200, 1.0), and (0, 0.9) on V = 4096 logits.

Per call (encode + decode + results on the host) at 128 sources x 8 samples and 1024 x 1: casv_decode_sample of this build, of the
parent commit's build (--parent-lib: its libcor_asv_ann_hip.so, loaded through CASV_LIB_PATH) and casv_decode_sample_cut at
top_p = 0.9.  The only requirement is on the first two: equal within the larger of their spreads ("plain_equals_parent").

Section 5's conventions: a process per series, the series alternating over RUNS runs, per run >= 100 ms of the same call as warm-up,
then the median of CALLS calls; "spread" = largest minus smallest of a series' run medians.

    python profiles/sample_cut.py --parent-lib PATH [--out FILE] [--commit ID]
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEPTH, WIDTH, VOC, SOURCES, SAMPLES, LENGTH, ROWS = 4, 512, 256, 128, 8, 100, 1024
CALLS, RUNS = 5, 3
LAUNCHES = (('sample_kernel_k0', VOC, None, 0, 1.0), ('sample_kernel_k64', VOC, None, 64, 1.0),
            ('sample_cut_kernel_p0.9', VOC, True, 0, 0.9), ('sample_cut_kernel_k64', VOC, True, 64, 1.0),
            ('sample_cut_kernel_k200', VOC, True, 200, 1.0), ('sample_cut_kernel_p0.9_V4096', 4096, True, 0, 0.9))


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


def series(name):
    """One series in this process: a JSON line {key: figure}."""
    from cor_asv_ann_amd.engine import HipEngine
    from cor_asv_ann_amd.synthetic import ModelConfig, make_weights, make_lines
    if name == 'launches':
        eng = HipEngine(1, 32, 40)
        rng = np.random.default_rng(1)
        out = {}
        for key, V, cut, top_k, top_p in LAUNCHES:
            x = (rng.standard_normal((ROWS, V)) * 3).astype(np.float32)
            call = (lambda: eng.debug_sample_cut_rows(x, 1.0, top_k, top_p, seed=1)) if cut else (lambda: eng.debug_sample_rows(x, 1.0, top_k, seed=1))
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.1:
                call()
            eng.profile(True)
            for _ in range(CALLS):
                call()
            p = eng.profile_read('sample')
            eng.profile(False)
            out[key] = 1e3 * p['ms'] / max(int(p['launches']), 1)          # us per launch
        eng.close()
        return out
    cfg = ModelConfig(depth=DEPTH, width=WIDTH, voc_size=VOC)
    _, sidx = make_lines(ROWS, LENGTH - 1, 104, voc_size=VOC)
    eng = HipEngine(DEPTH, WIDTH, VOC)
    eng.set_weights(make_weights(cfg, emb_scale=4.0))
    eng.set_option('arithmetic', 2)
    eng.set_option('persistent', 0)

    def call(n_sources, n):
        def run():
            eng.encode(sidx[:n_sources])
            return eng.decode_sample_cut(n, top_p=0.9, seed=1) if name == 'cut' else eng.decode_sample(n, seed=1)
        return run
    out = {}
    for key, c in (('%dx%d' % (SOURCES, SAMPLES), call(SOURCES, SAMPLES)), ('%dx1' % ROWS, call(ROWS, 1))):
        c()
        out[key] = median_ms(c)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sample_cut.json'))
    ap.add_argument('--commit', default='')
    ap.add_argument('--parent-lib', default='')
    ap.add_argument('--series', default='')
    args = ap.parse_args()
    if args.series:
        print('SERIES ' + json.dumps(series(args.series)))
        return
    names = ['launches', 'plain', 'cut'] + (['parent'] if args.parent_lib else [])
    runs = {n: [] for n in names}
    for run in range(RUNS):
        for n in (names if run % 2 == 0 else names[::-1]):
            env = dict(os.environ)
            if n == 'parent':
                env['CASV_LIB_PATH'] = os.path.abspath(args.parent_lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--series', n], env=env, check=True, capture_output=True, text=True,
                               timeout=300)
            runs[n].append(json.loads([l for l in r.stdout.splitlines() if l.startswith('SERIES ')][-1][7:]))
    med = {n: {k: float(np.median([r[k] for r in rs])) for k in rs[0]} for n, rs in runs.items()}
    spread = {n: {k: float(max(r[k] for r in rs) - min(r[k] for r in rs)) for k in rs[0]} for n, rs in runs.items()}
    out = {'what': 'per launch (us, R = %d rows, class "sample" of casv_profile_read through the debug entries) and per call (ms: encode + '
                   'decode + results on the host; depth %d width %d V %d, %d positions, S = %d, arithmetic 2) of sampling with and without '
                   'a cut; plain = casv_decode_sample of this build, parent = of the parent commit\'s build, cut = casv_decode_sample_cut '
                   'at top_p 0.9; a process per series and run, %d runs alternating, 100 ms of warm-up, median of %d calls'
                   % (ROWS, DEPTH, WIDTH, VOC, LENGTH, 2 * LENGTH, RUNS, CALLS),
           'host': socket.gethostname(), 'commit': args.commit, 'runs': runs, 'median': med, 'spread': spread}
    if 'parent' in med:
        out['plain_equals_parent'] = {k: abs(med['plain'][k] - med['parent'][k]) <= max(spread['plain'][k], spread['parent'][k]) for k in med['plain']}
        out['plain_minus_parent_ms'] = {k: med['plain'][k] - med['parent'][k] for k in med['plain']}
    out['cut_over_plain'] = {k: med['cut'][k] / med['plain'][k] for k in med['plain']}
    print(json.dumps(out))
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
