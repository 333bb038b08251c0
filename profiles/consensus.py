"""What the vote costs: 512 sources x 16 candidates as sample_lines draws them at depth 4, width 512, V 256 from the lines of bench
config c3 (seed 103, 100 characters and the end of line; S = 202 steps).

kernels    -- casv_consensus on all 512 x 16 candidates in ONE call, class "consensus" of casv_profile_read (both kernels), and the
              wall time of that call (copies included); median of CALLS calls after >= 100 ms of the same call as warm-up.
whole call -- consensus_lines (n = 16, with and without the greedy candidate) against the sample_lines call it contains, same
              seed, batch_size 1024 (64 sources per chunk), one process, alternating; per run the median of CALLS calls after one
              warm-up call, RUNS runs each; "spread" = largest minus smallest run median.
host       -- Alignment.get_levenshtein_distance (the only edit distance the tree had) on the 120 pairs of each of the first
              HOST_SOURCES sources, scaled to all 512 x 120 pairs.

    python profiles/consensus.py [--out FILE] [--commit ID]
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

DEPTH, WIDTH, VOC, SOURCES, N, LENGTH, LINE_SEED, EMB_SCALE = 4, 512, 256, 512, 16, 100, 103, 128.0
CALLS, RUNS, HOST_SOURCES = 5, 3, 2


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'consensus.json'))
    ap.add_argument('--commit', default='')
    args = ap.parse_args()
    import logging
    from cor_asv_ann_amd.metrics import Alignment
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence
    from cor_asv_ann_amd.synthetic import ModelConfig, make_weights, make_lines, make_vocabulary
    cfg = ModelConfig(depth=DEPTH, width=WIDTH, voc_size=VOC)
    logger = logging.getLogger('consensus')
    logger.setLevel(logging.CRITICAL)
    s2s = Sequence2Sequence(logger=logger)
    s2s.depth, s2s.width, s2s.batch_size = DEPTH, WIDTH, 1024
    s2s.mapping, s2s.voc_size = make_vocabulary(VOC), VOC
    s2s.configure()
    s2s.set_weights(make_weights(cfg, emb_scale=EMB_SCALE))
    s2s.status = 2
    lines, _ = make_lines(SOURCES, LENGTH, LINE_SEED, voc_size=VOC)
    kw = dict(n=N, seed=1)

    cands = s2s.sample_lines(lines, **kw)[0]
    eng = s2s.engine
    L = max(len(c) for cs in cands for c in cs)
    sym = np.zeros((SOURCES, N, L), np.int32)
    length = np.empty((SOURCES, N), np.int32)
    for b, cs in enumerate(cands):
        for k, c in enumerate(cs):
            sym[b, k, :len(c)] = [ord(ch) for ch in c]
            length[b, k] = len(c)
    cells = int(sum(int(length[b, i]) * int(length[b, j]) for b in range(SOURCES) for i in range(N) for j in range(i + 1, N)))

    def vote():
        return eng.consensus(sym, length)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.1:
        vote()
    wall = [timed(vote) for _ in range(CALLS)]
    eng.profile(True)
    kernel = []
    for _ in range(CALLS):
        before = eng.profile_read('consensus')
        vote()
        after = eng.profile_read('consensus')
        assert after['launches'] == before['launches'] + 1
        kernel.append(after['ms'] - before['ms'])
    eng.profile(False)
    risk, pick, dist = eng.consensus(sym, length, want_dist=True)

    calls = {'sample_lines': lambda: s2s.sample_lines(lines, **kw),
             'consensus_lines': lambda: s2s.consensus_lines(lines, **kw),
             'consensus_lines_without_greedy': lambda: s2s.consensus_lines(lines, include_greedy=False, **kw)}
    medians = {k: [] for k in calls}
    for run in range(RUNS):
        for name in (list(calls) if run % 2 == 0 else list(calls)[::-1]):
            calls[name]()
            medians[name].append(float(np.median([timed(calls[name]) for _ in range(CALLS)])))
    med = {k: float(np.median(v)) for k, v in medians.items()}

    t0 = time.perf_counter()
    for b in range(HOST_SOURCES):
        for i in range(N):
            for j in range(i + 1, N):
                d, _ = Alignment.get_levenshtein_distance(cands[b][i], cands[b][j])
                assert d == dist[b, i, j]
    host_s = (time.perf_counter() - t0) * SOURCES / HOST_SOURCES
    s2s.engine.close()

    pairs = SOURCES * N * (N - 1) // 2
    out = {'what': 'the vote over %d sources x %d candidates drawn by sample_lines (depth %d, width %d, V %d, emb_scale %g, lines of bench '
                   'config c3: seed %d, %d characters and the end of line); see profiles/consensus.py' % (SOURCES, N, DEPTH, WIDTH, VOC, EMB_SCALE, LINE_SEED, LENGTH),
           'host': socket.gethostname(), 'commit': args.commit,
           'candidates': {'mean_length': float(length.mean()), 'min_length': int(length.min()), 'max_length': int(length.max()), 'pairs': pairs,
                          'dp_cells': cells, 'mean_distance': float(np.mean([dist[b][np.triu_indices(N, 1)].mean() for b in range(SOURCES)])),
                          'picks_of_candidate_0': int((pick == 0).sum())},
           'kernels_ms': {'calls': kernel, 'median': float(np.median(kernel)), 'cells_per_us': cells / (float(np.median(kernel)) * 1e3)},
           'call_wall_ms': {'calls': wall, 'median': float(np.median(wall))},
           'whole_call': {'run_medians_ms': medians, 'median_ms': med, 'spread_ms': {k: float(max(v) - min(v)) for k, v in medians.items()},
                          'consensus_over_sample': med['consensus_lines'] / med['sample_lines'],
                          'without_greedy_over_sample': med['consensus_lines_without_greedy'] / med['sample_lines']},
           'host_python': {'pairs_timed': HOST_SOURCES * N * (N - 1) // 2, 'scaled_to_all_pairs_s': host_s}}
    print(json.dumps(out))
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
