"""What the retrieval of the K likeliest characters costs behind a scoring call: score_targets alone against score_targets followed
by score_alternatives(K = 8).  Depth 4, width 512, V 256, 512 decoder rows x 100 characters (profiles/score_targets_timing.py's
arrays): the retrieval reads 512 x 102 = 52 224 rows of Vp floats once, selects, and copies 2 K + 1 numbers per row back.

One handle, one process, alternating: per run >= 100 ms of the same call as warm-up, then the median of CALLS calls; RUNS runs each.
"spread" = largest minus smallest of the plain runs' medians.  Also recorded: the retrieval alone (repeated after one scoring call),
with and without the entropy, and at K = 1 and 64.

    python profiles/score_alternatives_timing.py [--out FILE] [--commit ID]
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

DEPTH, WIDTH, VOC, R, LENGTH = 4, 512, 256, 512, 100
K = 8
CALLS, RUNS = 10, 3


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'score_alternatives.json'))
    ap.add_argument('--commit', default='')
    args = ap.parse_args()
    from cor_asv_ann_amd.engine import HipEngine
    from cor_asv_ann_amd.synthetic import ModelConfig, make_weights, make_lines
    cfg = ModelConfig(depth=DEPTH, width=WIDTH, voc_size=VOC)
    weights = make_weights(cfg, emb_scale=4.0)
    _, sidx = make_lines(R, LENGTH, 104, voc_size=VOC)
    rng = np.random.default_rng(1104)
    tidx = sidx.copy()
    sub = rng.random(tidx.shape) < 0.05
    sub[:, -1] = False
    tidx[sub] = rng.integers(2, VOC, size=int(sub.sum()))
    U = LENGTH + 2
    dec_in = np.full((R, U), -1, np.int32)
    dec_out = np.full((R, U), -1, np.int32)
    dec_in[:, 1:LENGTH + 2] = tidx
    dec_out[:, :LENGTH + 1] = tidx

    eng = HipEngine(DEPTH, WIDTH, VOC)
    eng.set_weights(weights)

    def plain():
        return eng.score_targets(sidx, None, dec_in, dec_out)

    def with_alternatives():
        scores = eng.score_targets(sidx, None, dec_in, dec_out)
        return scores, eng.score_alternatives(K)
    calls = {'score_targets': plain, 'score_targets_then_alternatives': with_alternatives}
    scores, alt = with_alternatives()
    medians = {k: [] for k in calls}
    for run in range(RUNS):
        for name in (list(calls) if run % 2 == 0 else list(calls)[::-1]):
            medians[name].append(median_ms(calls[name]))
    plain()
    alone = {'K=%d%s' % (k, '' if h else ', no entropy'): median_ms(lambda: eng.score_alternatives(k, want_entropy=h))
             for k, h in ((K, True), (K, False), (1, True), (64, True))}
    eng.close()
    a, b = np.array(medians['score_targets']), np.array(medians['score_targets_then_alternatives'])
    scored = dec_out >= 0
    out = {'what': 'score_targets alone against score_targets followed by score_alternatives(K=%d), depth %d width %d V %d, %d decoder '
                   'rows x %d characters; median of %d calls per run, %d runs each, alternating, 100 ms of warm-up per run'
                   % (K, DEPTH, WIDTH, VOC, R, LENGTH, CALLS, RUNS),
           'host': socket.gethostname(), 'commit': args.commit,
           'score_targets_ms': medians['score_targets'], 'score_targets_then_alternatives_ms': medians['score_targets_then_alternatives'],
           'median_score_targets_ms': float(np.median(a)), 'median_score_targets_then_alternatives_ms': float(np.median(b)),
           'score_targets_spread_ms': float(a.max() - a.min()),
           'with_alternatives_over_plain': float(np.median(b) / np.median(a)),
           'retrieval_alone_ms': alone, 'rows': int(R * U),
           'check': {'first_place_is_best': bool(np.array_equal(alt[0][:, :, 0], scores[1])),
                     'share_of_targets_among_the_k': float((scores[2][scored] < K).mean()),
                     'mean_entropy_nats': float(alt[2][scored].mean())}}
    print(json.dumps(out))
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
