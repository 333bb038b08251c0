"""Host-side cost of the decode entry points: two builds of the library alternating on one GPU, three runs each.

    python profiles/decode_phases_timing.py collect <parent's libcor_asv_ann_hip.so> profiles/decode_phases_timing.json
    python profiles/decode_phases_timing.py small          (one run of the small search, prints its median ms per call)

bench_c2 / bench_c3: bench.py --gpus 1 --workload c2 | c3 --steps 10 --warmup 3 --no-cpu-baseline (ms_per_step).
small_search: depth 2, width 256, 16 lines of 40 characters, N = 8, graph 0 -- the launches are short, so the host's share of a
step shows most; median of 20 calls after 3."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def small():
    import numpy as np
    from oracle import ModelConfig, make_weights
    from cor_asv_ann_amd.engine import HipEngine
    cfg = ModelConfig(depth=2, width=256, voc_size=64)
    eng = HipEngine(2, 256, 64)
    eng.set_weights(make_weights(cfg, emb_scale=16.0))
    eng.set_option('graph', 0)
    rng = np.random.default_rng(1)
    idx = rng.integers(2, 64, (16, 40)).astype(np.int32)
    idx[:, -1] = 1
    times = []
    for call in range(23):
        eng.encode(idx)
        eng.synchronize()
        t0 = time.perf_counter()
        eng.decode_beam(batch_size=8)
        times.append(1e3 * (time.perf_counter() - t0))
    eng.close()
    print(json.dumps({'ms_per_step': sorted(times[3:])[10]}))


def one(cmd, lib):
    env = dict(os.environ)
    if lib:
        env['CASV_LIB_PATH'] = lib
    out = subprocess.run(cmd, cwd=ROOT, env=env, check=True, timeout=300, stdout=subprocess.PIPE, universal_newlines=True).stdout
    line = [x for x in out.split('\n') if x.startswith('{')][-1]
    return json.loads(line)['ms_per_step']


def collect(parent_lib, path):
    bench = [sys.executable, 'bench.py', '--gpus', '1', '--steps', '10', '--warmup', '3', '--no-cpu-baseline', '--workload']
    runs = {'bench_c2_ms_per_step': bench + ['c2'], 'bench_c3_ms_per_step': bench + ['c3'],
            'small_search_ms_per_call': [sys.executable, os.path.abspath(__file__), 'small']}
    result = {'what': __doc__.split('\n\n')[0] + ' ' + __doc__.split('\n\n')[2].replace('\n', ' ')}
    for name, cmd in runs.items():
        r = {'parent': [], 'change': []}
        for rep in range(3):
            r['parent'].append(one(cmd, parent_lib))
            r['change'].append(one(cmd, None))
        med = lambda v: sorted(v)[1]
        r['parent_median'], r['parent_spread'] = med(r['parent']), max(r['parent']) - min(r['parent'])
        r['change_median'] = med(r['change'])
        r['change_minus_parent_median'] = r['change_median'] - r['parent_median']
        result[name] = r
        print(name, json.dumps(r), flush=True)
    with open(path, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    small() if sys.argv[1] == 'small' else collect(sys.argv[2], sys.argv[3])
