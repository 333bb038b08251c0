"""A sha256 per output of the train step's persistent FORWARD kernels (train_persist.hip, train_persist_top.hip: no atomics, so
their outputs are a function of the inputs), to compare two builds of the library bit for bit -- after profiles/train_state_bits.py.

    CASV_LIB_PATH=<a build's libcor_asv_ann_hip.so> python profiles/train_tile_bits.py OUT.json
    python profiles/train_tile_bits.py --compare A.json B.json [--unstable A2.json]

Cases: depth 2, V = 40, B = 33 (two row blocks, the second ragged), T = U = 3 at W = 128, 256, 512 -- NT = 4: the smallest width
at which all five kernels exist, every stage wait a full one; NT = 8: the smallest cell width with a counted wait; NT = 16: the
bench's.  A fourth case, W = 512 at B = 257 (nine row blocks, the last of one row): at W = 512 the launches around the recurrences
add split-K shares with atomics while the batch is small, so the B = 33 digests of logp, align and loss differ between two runs of
ONE build (measured: B = 33, 65, 129 differ, B = 257 repeats), and NT = 16 is compared bit for bit there.  Per case score_targets (log-probabilities, best and rank, alignments) outside a session and the loss of a mode-0
train_step inside one; "train_persistent_launches" must be > 0 behind each call, so the digests are the persistent kernels'.
The backward kernels add their K shares with float atomics: their bits are not defined across runs, and the noise bounds of
tests/test_gpu_train_forms.py hold them.  --unstable: a second collection of build A; a key that differs between A's own two
runs is named and left out of the comparison -- never a score_targets key (exit 1)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from profiles.train_state_bits import digest        # noqa: E402


def collect():
    from cor_asv_ann_amd.engine import HipEngine
    from tests import train_state_cases as tc
    out = {}
    for W, B in ((128, 33), (256, 33), (512, 33), (512, 257)):
        name, V = 'd2_w%d_b%d' % (W, B), 40
        w, batch = tc.weights_of(2, W, V, {}), tc.batch_of(V, B, 3, 3)
        eng = HipEngine(2, W, V)
        try:
            eng.set_weights(w)
            res = eng.score_targets(*batch[:4], want_align=True)
            assert eng.stat('train_persistent_launches') > 0, (name, 'score_targets ran per step')
            out[name + '/score_targets/logp'] = digest(res[0])
            out[name + '/score_targets/ranks'] = digest(res[1], res[2])
            out[name + '/score_targets/align'] = digest(res[5])
            eng.train_begin()
            loss, _ = eng.train_step(*batch, mode=0)
            assert eng.stat('train_persistent_launches') > 0, (name, 'the mode-0 step ran per step')
            out[name + '/train_step_mode0/loss'] = digest(np.float64(loss))
            eng.train_end()
        finally:
            eng.close()
    return out


def compare(a, b, a2=None):
    x, y = (json.load(open(p)) for p in (a, b))
    unstable = []
    if a2:
        x2 = json.load(open(a2))
        unstable = sorted(k for k in set(x) | set(x2) if x.get(k) != x2.get(k))
        for k in unstable:
            print('  differs between the first build\'s own two runs, left out:', k)
    keys = sorted(k for k in set(x) | set(y) if k not in unstable)
    bad = [k for k in keys if x.get(k) != y.get(k)]
    print('%d digests compared, %d differ' % (len(keys), len(bad)))
    for k in bad:
        print('  differs:', k)
    return 1 if bad or any('score_targets' in k for k in unstable) else 0


if __name__ == '__main__':
    if sys.argv[1] == '--compare':
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[5] if len(sys.argv) > 5 and sys.argv[4] == '--unstable' else None))
    result = collect()
    with open(sys.argv[1], 'w') as f:
        json.dump(result, f, indent=0, sort_keys=True)
        f.write('\n')
    print('%d digests -> %s' % (len(result), sys.argv[1]))
