"""What the confusion network costs: 512 sources x 16 candidates as sample_lines draws them at depth 4, width 512, V 256 from the
lines of bench config c3 (seed 103, 100 characters and the end of line; S = 202 steps) -- the inputs of profiles/consensus.py, drawn
by the model and not synthetic -- each source aligned to the candidate casv_consensus picks.

kernels    -- casv_consensus_align and casv_consensus_vote on all 512 x 16 candidates in ONE call each, and casv_consensus on the
              same arrays as the yardstick of the fill, all from class "consensus" of casv_profile_read; RUNS runs that take the
              three in alternating order, CALLS calls each per run after >= 100 ms of the same call as warm-up; the medians of the
              run medians.  The wall time of the calls (copies included) likewise.
fill/walk  -- with option "align_stamps" the shader clocks the waves spend in the fill and in the walk, summed over the waves: the
              shares of a wave's time, not of the kernel's (the waves overlap).
whole call -- confusion_of with the pivots given and with consensus_of picking them, batch_size 1024 (64 sources per chunk).
host       -- the numpy restatement of tests/align_cases.py (align_source and vote_source) on the first HOST_SOURCES sources,
              scaled to all 512; every device result of these sources is compared with it on the way.

    python profiles/confusion.py [--out FILE] [--commit ID]
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
CALLS, RUNS, HOST_SOURCES = 5, 3, 4


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def warm(call):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.1:
        call()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'confusion.json'))
    ap.add_argument('--commit', default='')
    args = ap.parse_args()
    import logging
    from ctypes import byref, c_int64
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence
    from cor_asv_ann_amd.synthetic import ModelConfig, make_weights, make_lines, make_vocabulary
    from tests import align_cases as ac
    cfg = ModelConfig(depth=DEPTH, width=WIDTH, voc_size=VOC)
    logger = logging.getLogger('confusion')
    logger.setLevel(logging.CRITICAL)
    s2s = Sequence2Sequence(logger=logger)
    s2s.depth, s2s.width, s2s.batch_size = DEPTH, WIDTH, 1024
    s2s.mapping, s2s.voc_size = make_vocabulary(VOC), VOC
    s2s.configure()
    s2s.set_weights(make_weights(cfg, emb_scale=EMB_SCALE))
    s2s.status = 2
    lines, _ = make_lines(SOURCES, LENGTH, LINE_SEED, voc_size=VOC)
    cands = s2s.sample_lines(lines, n=N, seed=1)[0]
    eng = s2s.engine
    L = max(len(c) for cs in cands for c in cs)
    sym = np.zeros((SOURCES, N, L), np.int32)
    length = np.empty((SOURCES, N), np.int32)
    for b, cs in enumerate(cands):
        for k, c in enumerate(cs):
            sym[b, k, :len(c)] = [ord(ch) for ch in c]
            length[b, k] = len(c)
    pivot = eng.consensus(sym, length)[1]
    where, ncol = eng.consensus_align(sym, length, pivot)
    C = int(ncol.max())
    src, mass, best = eng.consensus_vote(C)
    lp = length[np.arange(SOURCES), pivot].astype(np.int64)
    others = np.ones((SOURCES, N), bool)
    others[np.arange(SOURCES), pivot] = False
    cells = int((lp[:, None] * length * others).sum())
    dir_bytes = int((lp[:, None] * ((length + 31) // 32) * 8 * others).sum())
    walk_steps = int(((lp[:, None] + length) * others).sum())
    all_cells = int(sum(int(length[b, i]) * int(length[b, j]) for b in range(SOURCES) for i in range(N) for j in range(i + 1, N)))

    calls = {'align': lambda: eng.consensus_align(sym, length, pivot), 'vote': lambda: eng.consensus_vote(C),
             'consensus': lambda: eng.consensus(sym, length)}
    kernel = {k: [] for k in calls}
    wall = {k: [] for k in calls}
    for run in range(RUNS):
        for name in (list(calls) if run % 2 == 0 else list(calls)[::-1]):
            warm(calls[name])
            wall[name].append(float(np.median([timed(calls[name]) for _ in range(CALLS)])))
            eng.profile(True)
            ms = []
            for _ in range(CALLS):
                before = eng.profile_read('consensus')
                calls[name]()
                after = eng.profile_read('consensus')
                assert after['launches'] == before['launches'] + 1
                ms.append(after['ms'] - before['ms'])
            eng.profile(False)
            kernel[name].append(float(np.median(ms)))
        eng.consensus_align(sym, length, pivot)                  # (the vote of the next run reads this call's align)
    kmed = {k: float(np.median(v)) for k, v in kernel.items()}

    def stat(key):
        value = c_int64()
        assert eng.lib.casv_get_stat(eng.handle, key.encode(), byref(value)) == 0
        return value.value
    eng.set_option('align_stamps', 1)
    warm(calls['align'])
    stamped_ms, ticks = [], []
    eng.profile(True)
    for _ in range(CALLS):
        before = eng.profile_read('consensus')
        calls['align']()
        stamped_ms.append(eng.profile_read('consensus')['ms'] - before['ms'])
        ticks.append((stat('align_fill_ticks'), stat('align_walk_ticks')))
    eng.profile(False)
    eng.set_option('align_stamps', 0)
    fill, walk = (float(np.median([t[i] for t in ticks])) for i in (0, 1))

    facade = {'confusion_of_given_pivots': lambda: s2s.confusion_of(cands, pivots=pivot.tolist()),
              'confusion_of': lambda: s2s.confusion_of(cands),
              'consensus_of': lambda: s2s.consensus_of(cands)}
    fmed = {k: [] for k in facade}
    for run in range(RUNS):
        for name in (list(facade) if run % 2 == 0 else list(facade)[::-1]):
            facade[name]()
            fmed[name].append(float(np.median([timed(facade[name]) for _ in range(3)])))

    t0 = time.perf_counter()
    for b in range(HOST_SOURCES):
        w, n, s = ac.align_source(sym[b], length[b], int(pivot[b]))
        m, top = ac.vote_source(sym[b], length[b], s)
        assert np.array_equal(w, where[b]) and n == ncol[b] and np.array_equal(s, src[b, :n])
        assert np.array_equal(m.view(np.int64), mass[b, :n].view(np.int64)) and np.array_equal(top, best[b, :n])
    host_s = (time.perf_counter() - t0) * SOURCES / HOST_SOURCES
    s2s.engine.close()

    out = {'what': 'the confusion network of %d sources x %d candidates drawn by sample_lines (depth %d, width %d, V %d, emb_scale %g, lines of '
                   'bench config c3: seed %d, %d characters and the end of line), pivot = the pick of casv_consensus; see profiles/confusion.py'
                   % (SOURCES, N, DEPTH, WIDTH, VOC, EMB_SCALE, LINE_SEED, LENGTH),
           'host': socket.gethostname(), 'commit': args.commit,
           'candidates': {'mean_length': float(length.mean()), 'min_length': int(length.min()), 'max_length': int(length.max()),
                          'pairs_aligned': SOURCES * (N - 1), 'dp_cells_aligned': cells, 'direction_bytes': dir_bytes, 'walk_steps_at_most': walk_steps,
                          'pairs_of_the_distance_vote': SOURCES * N * (N - 1) // 2, 'dp_cells_of_the_distance_vote': all_cells,
                          'mean_ncol': float(ncol.mean()), 'max_ncol': C,
                          'mean_voted_classes_per_column': float((mass >= 0).sum() / max(int(ncol.sum()), 1))},
           'kernels_ms': {'run_medians': kernel, 'median': kmed,
                          'align_cells_per_us': cells / (kmed['align'] * 1e3), 'consensus_cells_per_us': all_cells / (kmed['consensus'] * 1e3),
                          'fill_estimate_from_the_yardstick_ms': kmed['consensus'] * cells / all_cells},
           'call_wall_ms': {'run_medians': wall, 'median': {k: float(np.median(v)) for k, v in wall.items()}},
           'align_stamps': {'kernel_ms_with_stamps': float(np.median(stamped_ms)), 'fill_ticks': fill, 'walk_ticks': walk,
                            'walk_share_of_wave_time': walk / max(fill + walk, 1.0)},
           'facade_ms': {'run_medians': fmed, 'median': {k: float(np.median(v)) for k, v in fmed.items()}},
           'host_numpy': {'sources_timed': HOST_SOURCES, 'scaled_to_all_sources_s': host_s}}
    print(json.dumps(out))
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
