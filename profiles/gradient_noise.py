"""Device train step against the float64 oracle in units of the fp32 oracle's noise, per case, path, deterministic setting and
tensor (tests/grad_noise_cases.py); the measurement behind C_RMS / C_MAX.  Also whether the old bound of tests/test_gpu_train.py
(2e-3 x max|grad| per tensor) sees the one-step mutations of tests/test_grad_noise_bounds.py.
    python profiles/gradient_noise.py OUT.txt"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import grad_noise_cases as gn  # noqa: E402


def main(out):
    lines, worst = [], [0.0, '', 0.0, '']
    for case in gn.ALL:
        cfg, w, inputs, batch = gn.build(case)
        o64, o32 = gn.oracle(cfg, w, inputs, np.float64, case[10]), gn.oracle(cfg, w, inputs, np.float32, case[10])
        for path in ('fused', 'stepwise'):
            for det in (0, 1):
                r = gn.ratios(gn.device(case, w, batch, path, det), o32, o64)
                for k, (a, b) in r.items():
                    if k in gn.ZERO_GRADIENTS:
                        lines.append('%-18s %-8s det=%d %-16s rms_ratio %8.3f max_ratio %8.3f (exact value 0: not bounded by ratio)' % (case[0], path, det, k, a, b))
                        continue
                    lines.append('%-18s %-8s det=%d %-16s rms_ratio %8.3f max_ratio %8.3f' % (case[0], path, det, k, a, b))
                    if a > worst[0]: worst[0], worst[1] = a, '%s %s det=%d %s' % (case[0], path, det, k)
                    if b > worst[2]: worst[2], worst[3] = b, '%s %s det=%d %s' % (case[0], path, det, k)
                print(lines[-1], flush=True)
        if case is not gn.MID:
            for name, got in gn.mutations(cfg, w, inputs, case[10]).items():
                r = gn.ratios(got, o32, o64)
                new = gn.excess(r)
                old = not all(gn.within_old_bound(got[2][k], o64[2][k], o64[1]) for k in o64[2])
                lines.append('%-18s mutation %-22s new_bound_excess %10.1f old_bound_catches %s' % (case[0], name, new, old))
    lines.append('largest rms_ratio %.3f (%s); largest max_ratio %.3f (%s)' % tuple(worst))
    with open(out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print(lines[-1])


if __name__ == '__main__':
    main(sys.argv[1])
