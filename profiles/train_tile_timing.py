"""The staged-tile refactor, timed: the parent's build of the library and this one alternating on one GPU (CASV_LIB_PATH), five runs
each of bench.py's train workload c4 -- the recipe and the functions of profiles/train_state_timing.py.

    python profiles/train_tile_timing.py <parent's libcor_asv_ann_hip.so> OUT.json

c4 is W = 512 alone: of the 29 instantiations it runs the five of NT = 16.  This build's mean must lie within the parent's own
run-to-run range of the parent's mean.  If it does not with the parent first in every pair, the pairs are run once more with this
build first (which build of a pair runs second is not part of the question) and both are reported."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from profiles.train_state_timing import one, save        # noqa: E402


def pairs(parent_lib, change_first):
    r = {'parent': [], 'change': []}
    for rep in range(5):
        for build in (('change', 'parent') if change_first else ('parent', 'change')):
            r[build].append(one(['--workload', 'c4'], parent_lib if build == 'parent' else None))
        print('c4', 'change first' if change_first else 'parent first', rep, r['parent'][-1], r['change'][-1], flush=True)
    r['parent_mean'], r['change_mean'] = sum(r['parent']) / 5, sum(r['change']) / 5
    r['parent_range'] = max(r['parent']) - min(r['parent'])
    r['within_parent_range'] = bool(abs(r['change_mean'] - r['parent_mean']) <= r['parent_range'])
    return r


if __name__ == '__main__':
    parent_lib, path = sys.argv[1], sys.argv[2]
    result = {'what': ' '.join(__doc__.split('\n\n')[0].split()), 'command': 'python bench.py --gpus 1 --steps 5 --warmup 2 --no-cpu-baseline --workload c4'}
    result['c4_ms_per_step'] = pairs(parent_lib, False)
    save(result, path)
    if not result['c4_ms_per_step']['within_parent_range']:
        result['c4_change_first_ms_per_step'] = pairs(parent_lib, True)
        save(result, path)
    sys.exit(0 if any(v['within_parent_range'] for k, v in result.items() if k.endswith('_ms_per_step')) else 1)
