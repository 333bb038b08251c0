"""score_targets against the mode-0 train step it shares its forward pass with, at BASELINE configs[3]'s shape: depth 4, width 512,
V 256, 512 pairs of 100 characters (bench.py's c4 arrays, without the masks).

Both calls run on one handle in one process, alternating: train_step(mode=0) inside a training session -- the parent commit's
path, which this commit leaves as it was -- and score_targets outside one (its own forward-only state).  Per run >= 100 ms of the
same call as warm-up (the clock's plateau), then the median of CALLS calls; RUNS runs each.  "spread" = largest minus
smallest of the mode-0 runs' medians.  Also recorded: lines/s, the persistent launches each call took, the device memory the
forward-only state holds next to a training session's (hipMemGetInfo differences around their first call at this shape), and
-- `--profile` -- the per-class kernel times of one call of each (casv_profile).

    python profiles/score_targets_timing.py [--out FILE] [--commit ID] [--profile]
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

DEPTH, WIDTH, VOC, B, LENGTH = 4, 512, 256, 512, 100
CALLS, RUNS = 10, 3
CLASSES = ('lstm_gemm', 'lstm_gemm_small', 'gemm', 'attention', 'softmax', 'beam', 'embed', 'persist')


def free_bytes():
    import torch
    torch.cuda.synchronize()
    return int(torch.cuda.mem_get_info()[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'score_targets_timing.json'))
    ap.add_argument('--commit', default='')
    ap.add_argument('--profile', action='store_true')
    args = ap.parse_args()
    from cor_asv_ann_amd.engine import HipEngine
    from cor_asv_ann_amd.synthetic import ModelConfig, make_weights, make_lines
    cfg = ModelConfig(depth=DEPTH, width=WIDTH, voc_size=VOC)
    weights = make_weights(cfg, emb_scale=4.0)
    _, sidx = make_lines(B, LENGTH, 104, voc_size=VOC)
    rng = np.random.default_rng(1104)
    tidx = sidx.copy()
    sub = rng.random(tidx.shape) < 0.05
    sub[:, -1] = False
    tidx[sub] = rng.integers(2, VOC, size=int(sub.sum()))
    U = LENGTH + 2
    dec_in = np.full((B, U), -1, np.int32)
    dec_out = np.full((B, U), -1, np.int32)
    dec_in[:, 1:LENGTH + 2] = tidx
    dec_out[:, :LENGTH + 1] = tidx
    wts = (dec_out >= 0).astype(np.float32)

    free_bytes()                                    # (the measuring context exists before the first reading)
    scorer = HipEngine(DEPTH, WIDTH, VOC)
    scorer.set_weights(weights)
    before = free_bytes()
    scored = scorer.score_targets(sidx, None, dec_in, dec_out)
    forward_only = before - free_bytes()
    trainer = HipEngine(DEPTH, WIDTH, VOC)
    trainer.set_weights(weights)
    before = free_bytes()
    trainer.train_begin()
    loss0 = trainer.train_step(sidx, None, dec_in, dec_out, wts, None, mode=0)[0]
    session_mode0 = before - free_bytes()
    trainer.train_step(sidx, None, dec_in, dec_out, wts, None, mode=1)
    session = before - free_bytes()
    trainer.train_end()
    trainer.train_begin()

    calls = {'mode0': lambda: trainer.train_step(sidx, None, dec_in, dec_out, wts, None, mode=0),
             'score': lambda: scorer.score_targets(sidx, None, dec_in, dec_out)}
    engines = {'mode0': trainer, 'score': scorer}
    medians = {k: [] for k in calls}
    launches = {}
    for run in range(RUNS):
        for name in (('mode0', 'score') if run % 2 == 0 else ('score', 'mode0')):
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
    m0, sc_ = np.array(medians['mode0']), np.array(medians['score'])
    spread = float(m0.max() - m0.min())
    out = {'what': 'score_targets against train_step(mode=0), depth %d width %d V %d, %d pairs x %d characters; median of %d calls per run, '
                   '%d runs each, alternating, 100 ms of warm-up per run' % (DEPTH, WIDTH, VOC, B, LENGTH, CALLS, RUNS),
           'host': socket.gethostname(), 'commit': args.commit,
           'mode0_ms': medians['mode0'], 'score_ms': medians['score'],
           'median_mode0_ms': float(np.median(m0)), 'median_score_ms': float(np.median(sc_)), 'mode0_spread_ms': spread,
           'score_minus_mode0_ms': float(np.median(sc_) - np.median(m0)),
           'score_within_mode0_plus_spread': bool(np.median(sc_) <= np.median(m0) + spread),
           'score_lines_per_s': B / (float(np.median(sc_)) * 1e-3), 'score_chars_per_s': B * (LENGTH + 1) / (float(np.median(sc_)) * 1e-3),
           'persistent_launches': launches,
           'forward_only_state_bytes': forward_only, 'training_session_bytes_after_mode0': session_mode0, 'training_session_bytes': session,
           'check': {'mode0_loss': loss0, 'mean_nll_per_char': float(scored[3].sum() / scored[4].sum())}}
    if args.profile:
        prof = {}
        for name in calls:
            eng = engines[name]
            eng.profile(1)
            calls[name]()
            eng.synchronize()
            prof[name] = {c: eng.profile_read(c) for c in CLASSES}
            prof[name] = {c: v for c, v in prof[name].items() if v['launches']}
            eng.profile(0)
        out['profile_one_call'] = prof
    trainer.train_end()
    trainer.close()
    scorer.close()
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps({k: v for k, v in out.items() if k != 'profile_one_call'}))


if __name__ == '__main__':
    main()
