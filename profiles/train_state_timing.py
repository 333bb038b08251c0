"""The training-state refactor, timed: the parent's build of the library and this one alternating on one GPU (CASV_LIB_PATH), five
runs each, on bench.py's train workload c4 and its default workload c3 (the pattern of profiles/encoder_table_timing.py); then
the wall time of HipEngine.train_gradients() on the depth-2 W = 256 model with either build.

    python profiles/train_state_timing.py <parent's libcor_asv_ann_hip.so> OUT.json [gradients | c4_change_first]

Every bench run is `python bench.py --gpus 1 --steps 5 --warmup 2 --no-cpu-baseline [--workload c4]`.  The step's launches are the
parent's, so the question is whether the host got slower: a workload's mean must lie within the parent's own run-to-run range of the
parent's mean.  `gradients`: only the train_gradients() part.  `c4_change_first`: OUT.json exists; c4 once more with this build
first in every pair (which build of a pair runs second is not part of the question), added to the file."""
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one(extra, lib=None):
    env = dict(os.environ)
    if lib:
        env['CASV_LIB_PATH'] = lib
    cmd = [sys.executable, 'bench.py', '--gpus', '1', '--steps', '5', '--warmup', '2', '--no-cpu-baseline'] + extra
    out = subprocess.run(cmd, cwd=ROOT, env=env, check=True, timeout=300, stdout=subprocess.PIPE, universal_newlines=True).stdout
    line = [x for x in out.split('\n') if x.startswith('{')][-1]
    return json.loads(line)['ms_per_step']


def gradients_ms():
    """Median wall time of train_gradients() behind one step, in this process's build (a child process per build)."""
    import numpy as np
    from cor_asv_ann_amd.engine import HipEngine
    from tests import train_state_cases as tc
    eng = HipEngine(2, 256, 40)
    eng.set_weights(tc.weights_of(2, 256, 40, {}))
    eng.train_begin()
    eng.train_step(*tc.batch_of(40, 4, 8, 8), mode=2)
    times = []
    for _ in range(7):
        t0 = time.perf_counter()
        g = eng.train_gradients()
        times.append(1e3 * (time.perf_counter() - t0))
    eng.train_end()
    eng.close()
    return {'tensors': len(g), 'ms': times, 'median_ms': float(np.median(times))}


def save(result, path):
    text = re.sub(r'\[\s+([^\[\]]*?)\s+\]', lambda m: '[' + ' '.join(m.group(1).split()) + ']', json.dumps(result, indent=1))     # (a run's list on one line)
    with open(path, 'w') as f:
        f.write(text + '\n')


def change_first(parent_lib, path):
    with open(path) as f:
        result = json.load(f)
    r = {'change': [], 'parent': []}
    for rep in range(5):
        r['change'].append(one(['--workload', 'c4']))
        r['parent'].append(one(['--workload', 'c4'], parent_lib))
        print('c4, change first', rep, r['change'][-1], r['parent'][-1], flush=True)
    r['parent_mean'], r['change_mean'] = sum(r['parent']) / 5, sum(r['change']) / 5
    r['parent_range'] = max(r['parent']) - min(r['parent'])
    result['c4_change_first_ms_per_step'] = r
    save(result, path)


def main(parent_lib, path, only_gradients=False):
    result = {'what': ' '.join(__doc__.split('\n\n')[0].split()), 'command': 'python bench.py --gpus 1 --steps 5 --warmup 2 --no-cpu-baseline [--workload c4]'}
    for name, extra in () if only_gradients else (('c4', ['--workload', 'c4']), ('c3', [])):
        r = {'parent': [], 'change': []}
        for rep in range(5):            # alternating, so that drift of the box falls on both alike
            r['parent'].append(one(extra, parent_lib))
            r['change'].append(one(extra))
            print(name, rep, r['parent'][-1], r['change'][-1], flush=True)
        r['parent_mean'], r['change_mean'] = sum(r['parent']) / 5, sum(r['change']) / 5
        r['parent_range'] = max(r['parent']) - min(r['parent'])
        r['within_parent_range'] = bool(abs(r['change_mean'] - r['parent_mean']) <= r['parent_range'])
        result[name + '_ms_per_step'] = r
        save(result, path)
    g = {}
    for build, lib in (('parent', parent_lib), ('change', None)):
        env = dict(os.environ)
        if lib:
            env['CASV_LIB_PATH'] = lib
        out = subprocess.run([sys.executable, os.path.abspath(__file__), '--gradients-child'], cwd=ROOT, env=env, check=True, timeout=300,
                             stdout=subprocess.PIPE, universal_newlines=True).stdout
        g[build] = json.loads([x for x in out.split('\n') if x.startswith('{')][-1])
    g['parent_over_change'] = g['parent']['median_ms'] / g['change']['median_ms']
    print('train_gradients', g, flush=True)
    result['train_gradients_d2_w256'] = g
    save(result, path)


if __name__ == '__main__':
    if sys.argv[1] == '--gradients-child':
        print(json.dumps(gradients_ms()))
    elif len(sys.argv) > 3 and sys.argv[3] == 'c4_change_first':
        change_first(sys.argv[1], sys.argv[2])
    else:
        main(sys.argv[1], sys.argv[2], len(sys.argv) > 3 and sys.argv[3] == 'gradients')
