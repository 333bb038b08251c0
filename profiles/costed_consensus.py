"""What weighted edit costs cost, on section 4.9's inputs: 512 sources x 16 candidates as sample_lines
draws them at depth 4, width 512, V 256 from the lines of bench config c3 (seed 103), cut to the costed calls' 2048 characters if
needed; every source's candidate 0 is its pivot.

plain   -- casv_consensus and casv_consensus_align of this build against another build's (--parent-lib: the parent commit's library),
           class "consensus" of casv_profile_read: the default instantiation is meant to be the code it was, so the two must agree
           within the runs' spread.
costed  -- casv_consensus_costed and casv_consensus_align_costed at costs (1, 1, 1) without keys and at EditCosts.graded() with keys, as
           ratios to the plain calls of the same worker.
bench   -- bench.py's default run (--no-cpu-baseline) on this build and on the parent's, alternating.

A library is loaded once per process, so every measurement is a worker process of its own (--worker): 100 ms of the same call as
warm-up, then the median of CALLS profiled calls; the builds alternate, RUNS runs each, the order turned round every run;
"spread" = largest minus smallest run median.  Without --parent-lib only this build is measured.

    python profiles/costed_consensus.py [--parent-lib FILE] [--out FILE] [--commit ID] [--no-bench]
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEPTH, WIDTH, VOC, SOURCES, N, LENGTH, LINE_SEED, EMB_SCALE = 4, 512, 256, 512, 16, 100, 103, 128.0
CALLS, RUNS, MAX_L = 7, 3, 2048
# the compiled kernels (hipcc -S of consensus_kernels.hip for gfx950): VGPRs, SGPRs, the inner loop's instructions from its header to
# the branch back (s_waitcnt and branches counted); LDS bytes of a wave at candidates of 200 characters
KERNELS = {'consensus_dist_kernel': {'vgpr': 64, 'sgpr': 60, 'scratch': 0, 'inner_loop_instructions': 26, 'lds_bytes_at_200': (3 * 200 + 256) * 4},
           'consensus_dist_costed_kernel': {'vgpr': 40, 'sgpr': 76, 'scratch': 0, 'inner_loop_instructions': 34, 'lds_bytes_at_200': (200 + 128) * 16},
           'consensus_align_kernel': {'vgpr': 54, 'sgpr': 78, 'scratch': 0, 'inner_loop_instructions': 37, 'lds_bytes_at_200': (3 * 200 + 256) * 4},
           'consensus_align_costed_kernel': {'vgpr': 42, 'sgpr': 85, 'scratch': 0, 'inner_loop_instructions': 46, 'lds_bytes_at_200': (200 + 128) * 16}}


def draw(path):
    """The candidates of section 4.9, as arrays in `path`."""
    import logging
    from cor_asv_ann_amd.edit_costs import EditCosts
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence
    from cor_asv_ann_amd.synthetic import ModelConfig, make_weights, make_lines, make_vocabulary
    logger = logging.getLogger('costed_consensus')
    logger.setLevel(logging.CRITICAL)
    s2s = Sequence2Sequence(logger=logger)
    s2s.depth, s2s.width, s2s.batch_size = DEPTH, WIDTH, 1024
    s2s.mapping, s2s.voc_size = make_vocabulary(VOC), VOC
    s2s.configure()
    s2s.set_weights(make_weights(ModelConfig(depth=DEPTH, width=WIDTH, voc_size=VOC), emb_scale=EMB_SCALE))
    s2s.status = 2
    lines, _ = make_lines(SOURCES, LENGTH, LINE_SEED, voc_size=VOC)
    cands = [[c[:MAX_L] for c in cs] for cs in s2s.sample_lines(lines, n=N, seed=1)[0]]
    s2s.engine.close()
    points, _ = s2s._vote_inputs(cands, None, MAX_L)
    chunk = list(range(SOURCES))
    sym, length, _ = s2s._vote_arrays(chunk, N, points, [None] * SOURCES)
    key = s2s._vote_keys(chunk, N, EditCosts.graded().keys_of(points))
    np.savez(path, sym=sym, key=key, length=length)


def worker(path):
    """This process's library on the arrays of `path`: {call: median kernel ms}."""
    from cor_asv_ann_amd.edit_costs import EditCosts
    from cor_asv_ann_amd.engine import HipEngine
    data = np.load(path)
    sym, key, length = data['sym'], data['key'], data['length']
    pivot = np.zeros(len(sym), np.int32)
    eng = HipEngine(1, 32, 12)
    calls = {'consensus': lambda: eng.consensus(sym, length), 'align': lambda: eng.consensus_align(sym, length, pivot)}
    if hasattr(eng.lib, 'casv_consensus_costed'):
        graded = EditCosts.graded()
        calls.update({'consensus_costed_unit': lambda: eng.consensus(sym, length, costs=(1, 1, 1, 1)),
                      'consensus_costed_graded': lambda: eng.consensus(sym, length, key=key, costs=graded),
                      'align_costed_unit': lambda: eng.consensus_align(sym, length, pivot, costs=(1, 1, 1, 1)),
                      'align_costed_graded': lambda: eng.consensus_align(sym, length, pivot, key=key, costs=graded)})
    out = {}
    for name, call in calls.items():
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.1:
            call()
        eng.profile(True)
        ms = []
        for _ in range(CALLS):
            before = eng.profile_read('consensus')
            call()
            after = eng.profile_read('consensus')
            assert after['launches'] == before['launches'] + 1
            ms.append(after['ms'] - before['ms'])
        eng.profile(False)
        out[name] = float(np.median(ms))
    eng.close()
    print('RESULT ' + json.dumps(out))


def child(argv, lib):
    env = dict(os.environ)
    if lib:
        env['CASV_LIB_PATH'] = lib
    else:
        env.pop('CASV_LIB_PATH', None)
    done = subprocess.run([sys.executable] + argv, env=env, cwd=ROOT, check=True, capture_output=True, text=True, timeout=600)
    print('done: %s on %s' % (os.path.basename(argv[0]), lib or 'this build'), file=sys.stderr, flush=True)
    return done.stdout


def summary(runs):
    return {'run_medians': runs, 'median': float(np.median(runs)), 'spread': float(max(runs) - min(runs))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'costed_consensus.json'))
    ap.add_argument('--commit', default='')
    ap.add_argument('--parent-lib', default='')
    ap.add_argument('--no-bench', action='store_true')
    ap.add_argument('--worker', default='')
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker)
    builds = ['this'] + (['parent'] if args.parent_lib else [])
    libs = {'this': '', 'parent': os.path.abspath(args.parent_lib) if args.parent_lib else ''}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'candidates.npz')
        draw(path)
        length = np.load(path)['length']
        runs = {b: {} for b in builds}
        for run in range(RUNS):
            for b in (builds if run % 2 == 0 else builds[::-1]):
                text = child([os.path.abspath(__file__), '--worker', path], libs[b])
                got = json.loads(next(line for line in text.splitlines() if line.startswith('RESULT '))[7:])
                for name, ms in got.items():
                    runs[b].setdefault(name, []).append(ms)
    kernels = {b: {name: summary(v) for name, v in runs[b].items()} for b in builds}
    this = kernels['this']
    ratios = {name: this[name]['median'] / this[name.split('_')[0]]['median'] for name in this if '_costed_' in name}
    bench = None
    if not args.no_bench:
        bench = {b: [] for b in builds}
        for run in range(RUNS - 1):
            for b in (builds if run % 2 == 0 else builds[::-1]):
                text = child([os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--no-cpu-baseline'], libs[b])
                bench[b].append(json.loads([line for line in text.splitlines() if line.startswith('{')][-1])['value'])
    out = {'what': 'weighted edit costs on %d sources x %d candidates drawn by sample_lines (depth %d, width %d, V %d, emb_scale %g, lines of '
                   'bench config c3: seed %d), candidate 0 as the pivot; see profiles/costed_consensus.py'
                   % (SOURCES, N, DEPTH, WIDTH, VOC, EMB_SCALE, LINE_SEED),
           'host': socket.gethostname(), 'commit': args.commit,
           'candidates': {'mean_length': float(length.mean()), 'min_length': int(length.min()), 'max_length': int(length.max())},
           'kernels_ms': kernels, 'costed_over_plain': ratios, 'compiled': KERNELS, 'bench_chars_per_s': bench}
    print(json.dumps(out))
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
