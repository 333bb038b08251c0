"""The measurements behind the minimum-risk head's test constants (run on an MI355X from the repository root):
    python profiles/risk_noise.py [output directory, default profiles/]
risk_head_noise.txt -- per head case of tests/risk_cases.py and padding value: the coefficients' and q's error in units of the
coefficient bound, the loss's and dlogits' error in units of the float32 head's own error (the noise unit); the largest noise
ratio is MEASURED_MAX_RATIO of tests/risk_cases.py, C is twice that, rounded up.
risk_noise.txt -- the whole mode-2 step on the two whole-step cases in the forms fused, stepwise and stepwise deterministic:
the largest rms and max ratios of tests/grad_noise_cases.py, with alpha beside them."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cor_asv_ann_amd.engine import HipEngine      # noqa: E402
from tests import grad_noise_cases as gn          # noqa: E402
from tests import risk_cases as rc                # noqa: E402
from tests import test_gpu_risk as tg             # noqa: E402


def main(out_dir):
    eng = HipEngine(1, 32, 40)
    worst = (0.0, None)
    worst_coef = 0.0
    with open(os.path.join(out_dir, 'risk_head_noise.txt'), 'w') as f:
        f.write('# case pad: coef / coefficient bound, q / coefficient bound, loss / noise unit, dlogits / noise unit\n')
        for case in rc.HEAD_CASES:
            for pad, (c_ratio, q_ratio, loss_ratio, d_ratio, _) in tg.head_figures(eng, case).items():
                f.write('V%d N%d G%d U%d pad %s: %.3g %.3g %.3f %.3f\n' % (case + (pad, c_ratio, q_ratio, loss_ratio, d_ratio)))
                f.flush()
                worst = max(worst, (loss_ratio, (case, pad, 'loss')), (d_ratio, (case, pad, 'dlogits')), key=lambda x: x[0])
                worst_coef = max(worst_coef, c_ratio, q_ratio)
        f.write('largest noise ratio %.3f at %r; largest share of the coefficient bound %.3g\n' % (worst[0], worst[1], worst_coef))
    eng.close()
    with open(os.path.join(out_dir, 'risk_noise.txt'), 'w') as f:
        f.write('# case form: largest rms ratio (quantity), largest max ratio (quantity); alpha %g; tests/grad_noise_cases.py has '
                'C_RMS %g, C_MAX %g\n' % (rc.STEP_ALPHA, gn.C_RMS, gn.C_MAX))
        for name in sorted(rc.STEP_CASES):
            for (path, det), (r, _, _) in tg.step_ratios(name).items():
                seen = {k: v for k, v in r.items() if k not in gn.ZERO_GRADIENTS}
                k_rms = max(seen, key=lambda k: seen[k][0])
                k_max = max(seen, key=lambda k: seen[k][1])
                f.write('%s %s det %d alpha %g: rms %.2f (%s), max %.2f (%s)\n' % (name, path, det, rc.STEP_ALPHA, seen[k_rms][0], k_rms,
                                                                                seen[k_max][1], k_max))
                f.flush()


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles'))
