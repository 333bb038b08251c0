"""The encoder's per-character table and the search's skipped last step, timed: the parent's build of the library and this one
alternating on one GPU (CASV_LIB_PATH) with this build's other stages in the same rounds -- the upper layers' input terms ahead
(CASV_ENCODER_TABLE=2), one stage off at a time (CASV_ENCODER_TABLE=0 / CASV_BEAM_SKIP_LAST=0), both off -- on bench.py's default
workload c3, five rounds; then the page workload both ways.

    python profiles/encoder_table_timing.py <parent's libcor_asv_ann_hip.so> OUT.json [verdict]

`verdict`: only the parent's build and this one, alternating, five runs each (the protocol of the verdict, nothing in between).

Every run is `python bench.py --gpus 1 --steps 5 --warmup 2 --no-cpu-baseline` (the defaults without the host baseline, which does
not touch ms_per_step).  The parent's range in the session is the noise; the change counts if its median is below the parent's by
more than three times that range."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(extra, lib=None, env_extra=None):
    env = dict(os.environ)
    if lib:
        env['CASV_LIB_PATH'] = lib
    env.update(env_extra or {})
    cmd = [sys.executable, 'bench.py', '--gpus', '1', '--steps', '5', '--warmup', '2', '--no-cpu-baseline'] + extra
    out = subprocess.run(cmd, cwd=ROOT, env=env, check=True, timeout=300, stdout=subprocess.PIPE, universal_newlines=True).stdout
    line = [x for x in out.split('\n') if x.startswith('{')][-1]
    return json.loads(line)['ms_per_step']


def median(v):
    s = sorted(v)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


STAGES = (('upper_layers_ahead_option_2', {'CASV_ENCODER_TABLE': '2'}), ('table_off_skip_on', {'CASV_ENCODER_TABLE': '0'}),
          ('table_on_skip_off', {'CASV_BEAM_SKIP_LAST': '0'}), ('both_off', {'CASV_ENCODER_TABLE': '0', 'CASV_BEAM_SKIP_LAST': '0'}))


def main(parent_lib, path, verdict_only=False):
    result = {'what': ' '.join(__doc__.split('\n\n')[0].split()), 'command': 'python bench.py --gpus 1 --steps 5 --warmup 2 --no-cpu-baseline'}
    c3 = {'parent': [], 'change': []}
    stages = {name: [] for name, _ in STAGES}
    for rep in range(5):            # one round = every variant once, so that drift of the box falls on all of them alike
        c3['parent'].append(one([], parent_lib))
        c3['change'].append(one([]))
        for name, env in STAGES if not verdict_only else ():
            stages[name].append(one([], None, env))
        print('c3', rep, c3['parent'][-1], c3['change'][-1], [v[-1] for v in stages.values() if v], flush=True)
    c3['parent_median'], c3['change_median'] = median(c3['parent']), median(c3['change'])
    c3['parent_range'] = max(c3['parent']) - min(c3['parent'])
    c3['change_minus_parent'] = c3['change_median'] - c3['parent_median']
    c3['counts'] = bool(c3['change_minus_parent'] < -3 * c3['parent_range'])
    result['c3_ms_per_step'] = c3
    if verdict_only:
        save(result, path)
        return
    result['c3_stages_ms_per_step'] = stages
    result['c3_stages_median'] = {name: median(v) for name, v in stages.items()}
    ahead = result['c3_stages_median']['upper_layers_ahead_option_2'] - c3['change_median']
    result['stage_c_upper_layers_ahead'] = {
        'option_2_minus_option_1_ms': ahead,
        'kept_as_default': bool(ahead < -c3['parent_range']),
        'rule': 'option 2 becomes the default only if its median is below option 1 (the change) by more than the parent\'s range'}
    save(result, path)
    page = {'parent': [], 'change': []}
    for rep in range(3):
        page['parent'].append(one(['--workload', 'page'], parent_lib))
        page['change'].append(one(['--workload', 'page']))
    page['parent_median'], page['change_median'] = median(page['parent']), median(page['change'])
    print('page', page, flush=True)
    result['page_ms_per_step'] = page
    save(result, path)


def save(result, path):
    with open(path, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2], len(sys.argv) > 3 and sys.argv[3] == 'verdict')
