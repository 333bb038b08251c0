"""What the minimum-risk head costs in the train step, and what a whole slice of minimum-risk training costs.  The README's
train-step shape: depth 4, width 512, V 256, 512 rows x 100 characters, as G = 64 groups of N = 8 candidates.

  hard step        casv_train_step (mode 1), on this build and -- with --parent-lib -- on a build of the parent commit
  risk step        casv_train_step_risk (mode 1) on the same arrays, with costs in [0, 1) and every eighth line not a member
  slice            training.risk_step on 64 sources x 8 candidates with a private proposal of the same shape: the proposal's
                   sample_lines (7 per source), consensus_of(distances=True) over the 64 sets, the host's lists (duplicates,
                   costs, vectorising) and the step

Every measurement is a process of its own, the processes alternate (parent, this build, risk, parent, ...); in a process per run
>= 100 ms of the same call as warm-up, then the median of CALLS calls, RUNS runs.  "spread" = largest minus smallest of a series'
medians.  The loss heads' kernel time comes from casv_profile (class "softmax", three steps each).

    python profiles/risk_step.py [--out FILE] [--commit ID] [--parent-lib FILE]
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
N = 8
ALPHA = 0.5
CALLS, RUNS, ROUNDS = 6, 3, 2


def median_ms(call, calls=CALLS):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.1:
        call()
    ts = []
    for _ in range(calls):
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
    cost = np.random.default_rng(7).random(B).astype(np.float32)
    cost[N - 1::N] = -1.0
    return sidx, dec_in, dec_out, w, cost


def engine():
    from cor_asv_ann_amd.engine import HipEngine
    from cor_asv_ann_amd.synthetic import ModelConfig, make_weights
    eng = HipEngine(DEPTH, WIDTH, VOC)
    eng.set_weights(make_weights(ModelConfig(depth=DEPTH, width=WIDTH, voc_size=VOC), emb_scale=4.0))
    eng.train_begin()
    return eng


def child(what):
    """One measurement in this process; prints one JSON line."""
    import cor_asv_ann_amd._native as nv
    if os.environ.get('CASV_LIB_PATH'):             # (a build of the parent commit has no risk entry point)
        nv.SIGNATURES.pop('casv_train_step_risk', None)
    sidx, dec_in, dec_out, w, cost = batch()
    out = {}
    if what == 'hard':
        eng = engine()
        out['ms'] = [median_ms(lambda: eng.train_step(sidx, None, dec_in, dec_out, w, None, mode=1)) for _ in range(RUNS)]
        eng.train_end()
        eng.close()
    elif what == 'risk':
        eng = engine()
        out['ms'] = [median_ms(lambda: eng.train_step_risk(sidx, None, dec_in, dec_out, w, cost, N, ALPHA, None, mode=1)) for _ in range(RUNS)]
        prof = {}
        for name, call in (('hard', lambda: eng.train_step(sidx, None, dec_in, dec_out, w, None, mode=1)),
                           ('risk', lambda: eng.train_step_risk(sidx, None, dec_in, dec_out, w, cost, N, ALPHA, None, mode=1))):
            eng.profile(1)
            for _ in range(3):
                call()
            prof[name] = eng.profile_read('softmax')           # (the loss head's launches)
            eng.profile(0)
        out['profile'] = prof
        eng.train_end()
        eng.close()
    elif what == 'slice':
        from cor_asv_ann_amd import training
        from cor_asv_ann_amd.seq2seq import Sequence2Sequence
        from cor_asv_ann_amd.synthetic import ModelConfig, make_lines, make_vocabulary, make_weights
        lines, _ = make_lines(B // N, LENGTH, 104, voc_size=VOC)
        s2s = Sequence2Sequence(progbars=False)
        s2s.depth, s2s.width, s2s.batch_size, s2s.dropout = DEPTH, WIDTH, B, 0.2
        s2s.mapping, s2s.voc_size = make_vocabulary(VOC), VOC
        s2s.configure()
        s2s.set_weights(make_weights(ModelConfig(depth=DEPTH, width=WIDTH, voc_size=VOC), emb_scale=4.0))
        s2s.status = 2
        proposal = training.proposal_copy(s2s)
        proposal.set_weights(s2s.get_weights())
        eng = s2s._require_engine()
        eng.train_begin()
        settings = {'samples': N, 'alpha': ALPHA, 'temperature': 1.0, 'top_k': 0, 'top_p': 1.0, 'seed': 5, 'own_proposal': True,
                    'model': s2s, 'batch_size': B, 'stream': 0}
        rng = np.random.default_rng(3)
        src, tgt = list(lines), list(lines)
        streams = list(range(len(src)))
        drawn = proposal.sample_lines(src, None, n=N - 1, seed=5, streams=streams)[0]
        cands = [[g] + list(d) for g, d in zip(tgt, drawn)]
        out['ms'] = [median_ms(lambda: training.risk_step(eng, proposal, (src, None, tgt), settings, rng), calls=3) for _ in range(RUNS)]
        out['sampling_ms'] = median_ms(lambda: proposal.sample_lines(src, None, n=N - 1, seed=5, streams=streams), calls=3)
        out['distances_ms'] = median_ms(lambda: proposal.consensus_of(cands, distances=True), calls=3)
        both = median_ms(lambda: training.risk_candidates(proposal, src, None, tgt, settings, 0), calls=3)
        out['candidates_ms'] = both
        out['lists_ms'] = both - out['sampling_ms'] - out['distances_ms']       # (duplicates and costs on the host)
        out['mean_candidate_length'] = float(np.mean([len(c) for cs in cands for c in cs]))
        eng.train_end()
        proposal.engine.close()
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'risk_step.json'))
    ap.add_argument('--commit', default='')
    ap.add_argument('--parent-lib', default='')
    ap.add_argument('--child', default='')
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    series = {'hard_parent': [], 'hard': [], 'risk': []}
    profile = None
    for _ in range(ROUNDS):
        if args.parent_lib:
            series['hard_parent'] += run_child('hard', os.path.abspath(args.parent_lib))['ms']
        series['hard'] += run_child('hard')['ms']
        risk = run_child('risk')
        series['risk'] += risk['ms']
        profile = risk['profile']
    whole = run_child('slice')
    med = {k: float(np.median(v)) for k, v in series.items() if v}
    out = {'what': 'train step (mode 1) with the cross-entropy and with the minimum-risk head (G = %d, N = %d), depth %d width %d V %d, '
                   '%d rows x %d characters; a slice of minimum-risk training on %d sources; median of %d calls per run, %d runs per '
                   'process, %d processes per series, alternating, 100 ms of warm-up per run'
                   % (B // N, N, DEPTH, WIDTH, VOC, B, LENGTH, B // N, CALLS, RUNS, ROUNDS),
           'host': socket.gethostname(), 'commit': args.commit,
           'ms': series, 'median_ms': med, 'spread_ms': {k: float(max(v) - min(v)) for k, v in series.items() if v},
           'risk_over_hard': med['risk'] / med['hard'],
           'hard_over_parent': med['hard'] / med['hard_parent'] if 'hard_parent' in med else None,
           'profile_of_three_steps': profile, 'slice': whole}
    print(json.dumps(out))
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
