"""score_candidates against score_targets on the same replicated pairs: what one encoder pass per source buys.  Depth 4, width 512,
V 256, 512 decoder rows x 100 characters (profiles/score_targets_timing.py's arrays), at (sources, candidates per source) =
(512, 1), (128, 4), (32, 16), (8, 64).

Per point two fresh handles in one process, alternating: score_targets on the 512 pairs with every source repeated once per
candidate -- the parent commit's way of rescoring, which this commit leaves as it was -- and score_candidates on the sources and the
same 512 targets.  Per run >= 100 ms of the same call as warm-up, then the median of CALLS calls; RUNS runs each.  "spread" = largest
minus smallest of the replicated runs' medians.  Also recorded per point: the persistent launches each call took, the device memory
each handle's forward-only state holds (hipMemGetInfo differences around its first call), and the per-class kernel times of one call
of each (casv_profile).  Conditions: at (512, 1) the two are the same launches -- within the spread; at no point is score_candidates
slower than the replicated call by more than the spread.

    python profiles/score_candidates_timing.py [--out FILE] [--commit ID]
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
POINTS = ((512, 1), (128, 4), (32, 16), (8, 64))
CALLS, RUNS = 10, 3
CLASSES = ('lstm_gemm', 'lstm_gemm_small', 'gemm', 'attention', 'softmax', 'beam', 'embed', 'persist')


def free_bytes():
    import torch
    torch.cuda.synchronize()
    return int(torch.cuda.mem_get_info()[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'score_candidates_timing.json'))
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

    free_bytes()                                    # (the measuring context exists before the first reading)
    points = []
    for Be, N in POINTS:
        src = np.ascontiguousarray(sidx[:Be])
        rep = np.ascontiguousarray(np.repeat(src, N, axis=0))
        din, dout = dec_in.reshape(Be, N, U), dec_out.reshape(Be, N, U)
        engines, state_bytes, first = {}, {}, {}
        calls = {'replicated': lambda: engines['replicated'].score_targets(rep, None, dec_in, dec_out),
                 'candidates': lambda: engines['candidates'].score_candidates(src, None, din, dout)}
        for name in calls:
            engines[name] = HipEngine(DEPTH, WIDTH, VOC)
            engines[name].set_weights(weights)
            before = free_bytes()
            first[name] = calls[name]()
            state_bytes[name] = before - free_bytes()
        medians = {k: [] for k in calls}
        launches = {}
        for run in range(RUNS):
            for name in (('replicated', 'candidates') if run % 2 == 0 else ('candidates', 'replicated')):
                t0 = time.perf_counter()
                while time.perf_counter() - t0 < 0.1:
                    calls[name]()
                ts = []
                for _ in range(CALLS):
                    t0 = time.perf_counter()
                    calls[name]()
                    ts.append(time.perf_counter() - t0)
                medians[name].append(float(np.median(ts)) * 1e3)
                launches[name] = engines[name].stat('train_persistent_launches')
        prof = {}
        for name in calls:
            eng = engines[name]
            eng.profile(1)
            calls[name]()
            eng.synchronize()
            prof[name] = {c: eng.profile_read(c) for c in CLASSES}
            prof[name] = {c: v for c, v in prof[name].items() if v['launches']}
            eng.profile(0)
        for eng in engines.values():
            eng.close()
        rp, cd = np.array(medians['replicated']), np.array(medians['candidates'])
        spread = float(rp.max() - rp.min())
        a, b = first['replicated'], first['candidates']
        points.append({
            'sources': Be, 'candidates_per_source': N,
            'replicated_ms': medians['replicated'], 'candidates_ms': medians['candidates'],
            'median_replicated_ms': float(np.median(rp)), 'median_candidates_ms': float(np.median(cd)), 'replicated_spread_ms': spread,
            'candidates_over_replicated': float(np.median(cd) / np.median(rp)),
            'not_slower_than_replicated_plus_spread': bool(np.median(cd) <= np.median(rp) + spread),
            'within_spread': bool(abs(np.median(cd) - np.median(rp)) <= spread),
            'persistent_launches': launches, 'forward_only_state_bytes': state_bytes, 'profile_one_call': prof,
            'check': {'largest_logp_difference': float(np.abs(a[0].reshape(-1) - b[0].reshape(-1)).max()),
                      'mean_nll_per_char': float(b[3].sum() / b[4].sum())}})
        print(json.dumps({k: v for k, v in points[-1].items() if k != 'profile_one_call'}))
    out = {'what': 'score_candidates against score_targets on the replicated pairs, depth %d width %d V %d, %d decoder rows x %d '
                   'characters; median of %d calls per run, %d runs each, alternating, 100 ms of warm-up per run'
                   % (DEPTH, WIDTH, VOC, R, LENGTH, CALLS, RUNS),
           'host': socket.gethostname(), 'commit': args.commit, 'points': points,
           'same_launches_point_within_spread': bool(points[0]['within_spread']),
           'no_point_slower_than_replicated_plus_spread': bool(all(p['not_slower_than_replicated_plus_spread'] for p in points))}
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
