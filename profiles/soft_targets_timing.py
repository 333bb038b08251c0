"""What soft targets cost in the train step, and what a distillation batch costs.  The README's train-step shape: depth 4, width
512, V 256, 512 lines x 100 characters.

  hard step        casv_train_step (mode 1), on this build and -- with --parent-lib -- on a build of the parent commit
  soft step        casv_train_step_soft (mode 1) at K = 8 on the same batch: the hard target with 0.5, seven others sharing 0.5
  distillation     a full batch of train(teacher=...): the depth-4 width-512 teacher scores the batch (score_targets), its 8
                   likeliest characters per position (score_alternatives) become 9-slot lists (alternatives_to_soft_targets) and
                   the depth-2 width-256 student takes the soft step; beside it the student's hard step alone

Every measurement is a process of its own (one handle each, at most two at a time: teacher and student), the processes alternate
(parent, this build, parent, ...); in a process per run >= 100 ms of the same call as warm-up, then the median of CALLS calls, RUNS
runs.  "spread" = largest minus smallest of a series' medians.  The loss head's kernel time comes from casv_profile (class
"softmax", three steps each); what the soft step costs beyond it is the host's check and upload of the lists.

    python profiles/soft_targets_timing.py [--out FILE] [--commit ID] [--parent-lib FILE]
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
STUDENT_DEPTH, STUDENT_WIDTH = 2, 256
K = 8
CALLS, RUNS, ROUNDS = 6, 3, 2


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
    soft_idx = np.full((B, U, K), -1, np.int32)
    soft_q = np.zeros((B, U, K), np.float32)
    others = (dec_out[:, :, None] + rng.integers(1, VOC // K, size=(B, U, K - 1)).cumsum(axis=2)) % VOC       # distinct, none the target
    scored = dec_out >= 0
    soft_idx[scored] = np.concatenate([dec_out[:, :, None], others], axis=2)[scored]
    soft_q[scored] = np.array([0.5] + [0.5 / (K - 1)] * (K - 1), np.float32)
    return sidx, dec_in, dec_out, w, soft_idx, soft_q


def engine(depth, width, training=True):
    from cor_asv_ann_amd.engine import HipEngine
    from cor_asv_ann_amd.synthetic import ModelConfig, make_weights
    eng = HipEngine(depth, width, VOC)
    eng.set_weights(make_weights(ModelConfig(depth=depth, width=width, voc_size=VOC), emb_scale=4.0))
    if training:
        eng.train_begin()
    return eng


def child(what):
    """One measurement in this process; prints one JSON line."""
    import cor_asv_ann_amd._native as nv
    if os.environ.get('CASV_LIB_PATH'):             # (a build of the parent commit has no soft entry points)
        nv.SIGNATURES.pop('casv_train_step_soft', None)
    sidx, dec_in, dec_out, w, soft_idx, soft_q = batch()
    out = {}
    if what == 'hard':
        eng = engine(DEPTH, WIDTH)
        out['ms'] = [median_ms(lambda: eng.train_step(sidx, None, dec_in, dec_out, w, None, mode=1)) for _ in range(RUNS)]
    elif what == 'soft':
        eng = engine(DEPTH, WIDTH)
        out['ms'] = [median_ms(lambda: eng.train_step_soft(sidx, None, dec_in, soft_idx, soft_q, w, None, mode=1)) for _ in range(RUNS)]
        prof = {}
        for name, call in (('hard', lambda: eng.train_step(sidx, None, dec_in, dec_out, w, None, mode=1)),
                           ('soft', lambda: eng.train_step_soft(sidx, None, dec_in, soft_idx, soft_q, w, None, mode=1))):
            eng.profile(1)
            for _ in range(3):
                call()
            prof[name] = eng.profile_read('softmax')           # (the loss head's launches)
            eng.profile(0)
        out['profile'] = prof
    elif what == 'distill':
        from cor_asv_ann_amd.seq2seq import alternatives_to_soft_targets
        teacher, eng = engine(DEPTH, WIDTH, training=False), engine(STUDENT_DEPTH, STUDENT_WIDTH)

        def scoring():
            teacher.score_targets(sidx, None, dec_in, dec_out)
            return teacher.score_alternatives(K, want_entropy=False)

        def lists():
            return alternatives_to_soft_targets(alt[0], alt[1], dec_out, alpha=0.5)

        def whole():
            a = scoring()
            si, sq = alternatives_to_soft_targets(a[0], a[1], dec_out, alpha=0.5)
            return eng.train_step_soft(sidx, None, dec_in, si, sq, w, None, mode=1)
        alt = scoring()
        si, sq = lists()
        out['ms'] = [median_ms(whole) for _ in range(RUNS)]
        out['teacher_scoring_ms'] = median_ms(scoring)
        out['lists_ms'] = median_ms(lists)
        out['student_soft_step_ms'] = median_ms(lambda: eng.train_step_soft(sidx, None, dec_in, si, sq, w, None, mode=1))
        out['student_hard_step_ms'] = median_ms(lambda: eng.train_step(sidx, None, dec_in, dec_out, w, None, mode=1))
        out['upload_bytes_per_step'] = int(si.nbytes + sq.nbytes)
        teacher.close()
    eng.train_end()
    eng.close()
    print('RESULT ' + json.dumps(out))


def run_child(what, lib=None):
    env = dict(os.environ)
    env.pop('CASV_LIB_PATH', None)
    if lib:
        env['CASV_LIB_PATH'] = lib
    res = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', what], env=env, check=True, timeout=600,
                         stdout=subprocess.PIPE, universal_newlines=True)
    return json.loads([ln for ln in res.stdout.splitlines() if ln.startswith('RESULT ')][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'soft_targets.json'))
    ap.add_argument('--commit', default='')
    ap.add_argument('--parent-lib', default='')
    ap.add_argument('--child', default='')
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    series = {'hard_parent': [], 'hard': [], 'soft': []}
    profile = None
    for _ in range(ROUNDS):
        if args.parent_lib:
            series['hard_parent'] += run_child('hard', args.parent_lib)['ms']
        series['hard'] += run_child('hard')['ms']
        soft = run_child('soft')
        series['soft'] += soft['ms']
        profile = soft['profile']
    distill = run_child('distill')
    med = {k: float(np.median(v)) for k, v in series.items() if v}
    out = {'what': 'train step (mode 1) on hard and on soft targets (K = %d), depth %d width %d V %d, %d lines x %d characters; a '
                   'distillation batch: that model as teacher, a depth-%d width-%d student; median of %d calls per run, %d runs per '
                   'process, %d processes per series, alternating, 100 ms of warm-up per run'
                   % (K, DEPTH, WIDTH, VOC, B, LENGTH, STUDENT_DEPTH, STUDENT_WIDTH, CALLS, RUNS, ROUNDS),
           'host': socket.gethostname(), 'commit': args.commit,
           'ms': series, 'median_ms': med, 'spread_ms': {k: float(max(v) - min(v)) for k, v in series.items() if v},
           'soft_over_hard': med['soft'] / med['hard'],
           'hard_over_parent': med['hard'] / med['hard_parent'] if 'hard_parent' in med else None,
           'profile_of_three_steps': profile, 'distillation_batch': distill}
    print(json.dumps(out))
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
