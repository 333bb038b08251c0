"""What scheduled sampling costs in the train step.  The README's train-step shape: depth 4, width 512, V 256, 512 lines x 100
characters, with dropout masks (rate 0.2).

  hard step          casv_train_step (mode 1), on this build and -- with --parent-lib -- on a build of the parent commit
  sampled step       casv_train_step_sampled (mode 1), greedy pick, ratio 0.5, at passes = 1 and passes = 2
  host composition   what a user could build without it, from entry points the feature leaves alone: score_targets (its `best` is
                     the greedy pick of every position), the mix on the host with numpy's generator, train_step on the mixed input

Every measurement is a process of its own (one handle each), the processes alternate (parent, this build, sampled, ...); in a
process per run >= 100 ms of the same call as warm-up, then the median of CALLS calls, RUNS runs.  "spread" = largest minus smallest
of a series' medians.  The kernel-class times of three steps come from casv_profile.

    python profiles/scheduled_sampling_timing.py [--out FILE] [--commit ID] [--parent-lib FILE]
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

DEPTH, WIDTH, VOC, B, LENGTH = 4, 512, 256, 512, 100
RATIO, DROPOUT = 0.5, 0.2
CALLS, RUNS, ROUNDS = 6, 3, 2
CLASSES = ('gemm', 'persist', 'softmax', 'sample')


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


def batch():
    from cor_asv_ann_amd.synthetic import make_lines
    _, sidx = make_lines(B, LENGTH, 104, voc_size=VOC)
    U = LENGTH + 2
    dec_in = np.full((B, U), -1, np.int32)
    dec_out = np.full((B, U), -1, np.int32)
    dec_in[:, 1:LENGTH + 2] = sidx
    dec_out[:, :LENGTH + 1] = sidx
    w = (dec_out >= 0).astype(np.float32)
    rng = np.random.default_rng(7)
    keep = lambda shape: ((rng.uniform(0, 1, shape) >= DROPOUT) / (1.0 - DROPOUT)).astype(np.float32)
    masks = {'enc': [keep(2 * WIDTH if n == 0 else WIDTH) for n in range(DEPTH)], 'dec': [keep(WIDTH) for _ in range(DEPTH - 1)],
             'cell': keep((B, 2 * WIDTH))}
    return sidx, dec_in, dec_out, w, masks


def child(what):
    """One measurement in this process; prints one JSON line."""
    import cor_asv_ann_amd._native as nv
    if os.environ.get('CASV_LIB_PATH'):             # (a build of the parent commit has no sampled entry points)
        nv.SIGNATURES.pop('casv_train_step_sampled', None)
    from cor_asv_ann_amd.engine import HipEngine
    from cor_asv_ann_amd.synthetic import ModelConfig, make_weights
    sidx, dec_in, dec_out, w, masks = batch()
    eng = HipEngine(DEPTH, WIDTH, VOC)
    eng.set_weights(make_weights(ModelConfig(depth=DEPTH, width=WIDTH, voc_size=VOC), emb_scale=4.0))
    eng.train_begin()
    step = [0]
    rng = np.random.default_rng(1)
    eligible = dec_in >= 0
    eligible[:, 0] = False

    def hard():
        return eng.train_step(sidx, None, dec_in, dec_out, w, masks, mode=1)

    def sampled(passes):
        step[0] += 1
        return eng.train_step_sampled(sidx, None, dec_in, dec_out, w, masks, mode=1, ratio=RATIO, seed=11, step_id=step[0], passes=passes)

    def host():
        best = eng.score_targets(sidx, None, dec_in, dec_out)[1]
        mixed = dec_in.copy()
        take = eligible & (rng.random(dec_in.shape) < RATIO)
        mixed[:, 1:][take[:, 1:]] = best[:, :-1][take[:, 1:]]          # (position u from the pick at u - 1)
        return eng.train_step(sidx, None, mixed, dec_out, w, masks, mode=1)

    call = {'hard': hard, 'sampled1': lambda: sampled(1), 'sampled2': lambda: sampled(2), 'host': host}[what]
    out = {'ms': [median_ms(call) for _ in range(RUNS)]}
    eng.profile(1)
    for _ in range(3):
        call()
    out['profile_of_three_steps'] = {c: eng.profile_read(c) for c in CLASSES}
    eng.profile(0)
    out['persistent_launches'] = eng.stat('train_persistent_launches') if hasattr(eng, 'stat') else None
    eng.train_end()
    eng.close()
    print('RESULT ' + json.dumps(out))


def run_child(what, lib=None):
    env = dict(os.environ)
    env.pop('CASV_LIB_PATH', None)
    if lib:
        env['CASV_LIB_PATH'] = lib
    res = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', what], env=env, check=True, timeout=300,
                         stdout=subprocess.PIPE, universal_newlines=True)
    return json.loads([ln for ln in res.stdout.splitlines() if ln.startswith('RESULT ')][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'scheduled_sampling.json'))
    ap.add_argument('--commit', default='')
    ap.add_argument('--parent-lib', default='')
    ap.add_argument('--child', default='')
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    series = {'hard_parent': [], 'hard': [], 'sampled_passes_1': [], 'sampled_passes_2': [], 'host_composition': []}
    profiles = {}
    for _ in range(ROUNDS):
        for name, what, lib in (('hard_parent', 'hard', args.parent_lib), ('hard', 'hard', None), ('sampled_passes_1', 'sampled1', None),
                                ('host_composition', 'host', None), ('sampled_passes_2', 'sampled2', None)):
            if name == 'hard_parent' and not lib:
                continue
            res = run_child(what, lib)
            series[name] += res['ms']
            profiles[name] = {'kernel_classes': res['profile_of_three_steps'], 'persistent_launches': res['persistent_launches']}
    med = {k: float(np.median(v)) for k, v in series.items() if v}
    spread = {k: float(max(v) - min(v)) for k, v in series.items() if v}
    out = {'what': 'train step (mode 1), depth %d width %d V %d, %d lines x %d characters, dropout %.1f: hard, sampled (greedy, ratio '
                   '%.1f) at 1 and 2 passes, and the host composition score_targets + host mix + train_step; median of %d calls per '
                   'run, %d runs per process, %d processes per series, alternating, 100 ms of warm-up per run'
                   % (DEPTH, WIDTH, VOC, B, LENGTH, DROPOUT, RATIO, CALLS, RUNS, ROUNDS),
           'host': socket.gethostname(), 'commit': args.commit,
           'ms': series, 'median_ms': med, 'spread_ms': spread,
           'hard_over_parent': med['hard'] / med['hard_parent'] if 'hard_parent' in med else None,
           'sampled_1_over_hard': med['sampled_passes_1'] / med['hard'], 'sampled_2_over_hard': med['sampled_passes_2'] / med['hard'],
           'host_composition_minus_sampled_1_ms': med['host_composition'] - med['sampled_passes_1'],
           'largest_spread_of_the_two_ms': max(spread['host_composition'], spread['sampled_passes_1']),
           'profile_of_three_steps': profiles}
    print(json.dumps(out))
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
