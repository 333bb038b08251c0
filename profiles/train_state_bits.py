"""A sha256 per output of the train step, the accessors and the scoring calls (a dict of tensors: one digest over its tensors'
digests), to compare two builds of the library bit for bit.

    CASV_LIB_PATH=<a build's libcor_asv_ann_hip.so> python profiles/train_state_bits.py OUT.json
    python profiles/train_state_bits.py --compare A.json B.json          (exit 1 and the differing keys unless all digests match)

Cases: the four topologies of tests/train_state_cases.py (W = 32, V = 7, B = 2, T = U = 3) and the depth-2 W = 64 case of
test_state_round_trip_continues_the_session.  Per case, "deterministic" on: weights, m, v, gradients, losses and norms after three
mode-1 steps and after one soft-target step (K = 2); score_targets, score_candidates (N = 2) and score_alternatives (K = 2)
outside a session; "deterministic" off: the same scoring outputs (scoring is a function of weights and line alone)."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def tensors(out, prefix, d):
    """One digest for a dict of tensors: over the tensors' own digests, by name."""
    out[prefix] = hashlib.sha256(''.join('%s:%s\n' % (k, digest(d[k])) for k in sorted(d)).encode()).hexdigest()


def session(out, prefix, eng, w, step):
    eng.set_weights(w)
    eng.train_begin()
    results = step(eng)
    out[prefix + '/loss_norm'] = digest(np.asarray(results, np.float64))
    tensors(out, prefix + '/grad', eng.train_gradients())
    m, v, count = eng.train_state()
    tensors(out, prefix + '/m', m)
    tensors(out, prefix + '/v', v)
    out[prefix + '/step'] = int(count)
    tensors(out, prefix + '/weights', eng.train_weights())
    eng.train_end()
    tensors(out, prefix + '/committed', eng.get_weights())


def scoring(out, prefix, eng, w, batch):
    eng.set_weights(w)
    sidx, val, di, do, _ = batch
    res = eng.score_targets(sidx, val, di, do, want_align=True)
    out[prefix + '/score_targets'] = digest(*res)
    out[prefix + '/score_alternatives'] = digest(*eng.score_alternatives(2))
    di2 = np.stack([di, np.roll(di, 1, axis=1)], axis=1)
    do2 = np.stack([do, np.roll(do, 1, axis=1)], axis=1)
    res = eng.score_candidates(sidx, val, di2, do2, want_align='sparse')
    out[prefix + '/score_candidates'] = digest(*(res[:5] + res[5]))
    out[prefix + '/score_candidates_alternatives'] = digest(*eng.score_alternatives(2))


def collect():
    from cor_asv_ann_amd.engine import HipEngine
    from tests import train_state_cases as tc
    from tests.test_gpu_deterministic_train import _small_case
    cases = [(name, depth, tc.W, tc.V, flags, tc.weights_of(depth, tc.W, tc.V, flags), tc.batch_of(tc.V, tc.B, tc.T, tc.U))
             for name, depth, flags in tc.CONFIGS]
    _, w, _, (sidx, val, di, do, wts, _) = _small_case(2, 64, 40, 6, 9)
    cases.append(('d2_w64_round_trip', 2, 64, 40, {}, w, (sidx, val, di, do, wts)))
    out = {}
    for name, depth, W, V, flags, w, batch in cases:
        soft = tc.soft_of(V, *batch[2].shape)
        eng = HipEngine(depth, W, V, **flags)
        try:
            eng.set_option('deterministic', 1)
            session(out, name + '/det/three_steps', eng, w, lambda e: [e.train_step(*batch, mode=1) for _ in range(3)])
            session(out, name + '/det/soft_step', eng, w,
                    lambda e: [e.train_step_soft(batch[0], batch[1], batch[2], soft[0], soft[1], batch[4], mode=1)])
            scoring(out, name + '/det', eng, w, batch)
            eng.set_option('deterministic', 0)
            scoring(out, name + '/plain', eng, w, batch)
        finally:
            eng.close()
    return out


def compare(a, b):
    with open(a) as f:
        x = json.load(f)
    with open(b) as f:
        y = json.load(f)
    bad = sorted(k for k in set(x) | set(y) if x.get(k) != y.get(k))
    print('%d digests, %d differ' % (len(set(x) | set(y)), len(bad)))
    for k in bad:
        print('  differs:', k)
    return 1 if bad else 0


if __name__ == '__main__':
    if sys.argv[1] == '--compare':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    result = collect()
    with open(sys.argv[1], 'w') as f:
        json.dump(result, f, indent=0, sort_keys=True)
        f.write('\n')
    print('%d digests -> %s' % (len(result), sys.argv[1]))
