"""Decode path against the float64 oracle in units of the fp32 oracle's noise, per case, arithmetic, step and quantity
(tests/decode_noise_cases.py); the measurement behind C_RMS / C_MAX.  Also the one-row mutations of tests/test_decode_noise_bounds.py:
their excess over the bound and whether the old per-step tolerance (rtol 2e-4, atol 2e-6) would have caught them.
    python profiles/decode_noise.py OUT.txt"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import decode_noise_cases as dn  # noqa: E402


def main(out):
    lines, worst = [], [0.0, '', 0.0, '']

    def record(where, r, nan_bad):
        for k, (a, b) in r.items():
            lines.append('%-40s %-8s rms_ratio %8.3f max_ratio %8.3f%s' % (where, k, a, b, ' NAN MISMATCH' if k in nan_bad else ''))
            if a > worst[0]: worst[0], worst[1] = a, '%s %s' % (where, k)
            if b > worst[2]: worst[2], worst[3] = b, '%s %s' % (where, k)
        print(lines[-1], flush=True)

    for case in dn.ENC_CASES:
        cfg, w, x, inputs = dn.build_encoder(case)
        o32, o64 = dn.oracle_encoder(cfg, w, x, np.float32), dn.oracle_encoder(cfg, w, x, np.float64)
        got = dn.device_encoder(case, w, inputs)
        record('enc %s' % case[0], dn.ratios(got, o32, o64), dn.nan_mismatch(got, o32))
    for case in dn.STEP_CASES:
        cfg, w, (line, enc, states, a, p_in) = dn.build_step(case)
        engs = {ar: dn.step_engine(cfg, w, enc, ar) for ar in (0, 2)}
        for s in range(case[7]):
            o32 = dn.oracle_step(cfg, w, line, enc, states, a, p_in, np.float32)
            o64 = dn.oracle_step(cfg, w, line, enc, states, a, p_in, np.float64)
            for ar, eng in engs.items():
                got = dn.device_step(eng, line, states, a, p_in)
                record('step %s arith=%d s=%d' % (case[0], ar, s), dn.ratios(got, o32, o64), dn.nan_mismatch(got, o32))
            states, a, p_in = dn.next_inputs(cfg, o32)
        for eng in engs.values():
            eng.close()
    cfg, w, inputs = dn.build_step(dn.STEP_CASES[0])
    o32, o64 = dn.oracle_step(cfg, w, *inputs, np.float32), dn.oracle_step(cfg, w, *inputs, np.float64)
    for name, got in dn.step_mutations(cfg, w, inputs, o64).items():
        lines.append('step %-28s mutation %-30s new_bound_excess %10.1f old_tolerance_catches %s'
                     % (dn.STEP_CASES[0][0], name, dn.excess(dn.ratios(got, o32, o64)), dn.old_catches(got, o64)))
    for case in dn.ENC_CASES[:1] + dn.ENC_CASES[5:6]:
        cfg, w, x, _ = dn.build_encoder(case)
        o32, o64 = dn.oracle_encoder(cfg, w, x, np.float32), dn.oracle_encoder(cfg, w, x, np.float64)
        for name, got in dn.encoder_mutations(cfg, w, x).items():
            lines.append('enc  %-28s mutation %-30s new_bound_excess %10.1f old_tolerance_catches %s'
                         % (case[0], name, dn.excess(dn.ratios(got, o32, o64)), dn.old_catches(got, o64)))
    lines.append('largest rms_ratio %.3f (%s); largest max_ratio %.3f (%s)' % tuple(worst))
    with open(out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines[-12:]))


if __name__ == '__main__':
    main(sys.argv[1])
