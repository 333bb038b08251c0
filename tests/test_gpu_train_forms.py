"""Every form of the train step's persistent recurrences against float64 (tests/train_form_cases.py): one mode-2 step per case on
the fused and on the stepwise path, loss, norm and every gradient tensor within C_RMS / C_MAX of the fp32 oracle's own noise
(tests/grad_noise_cases.py: constants and the rule for att_bv unchanged), the form the step took read back from the statistics
"train_persistent_launches" / "train_give_ups" and compared with train_form's prediction for the device's CUs, and a mask-free
mode-0 evaluation behind it held to the oracle's loss_ce in the same unit.  tests/test_train_form_cases.py shows without a GPU that
the table reaches every instantiation and that the bounds see a leaking row clamp or a job cut short.

The suite is run with and without CASV_POISON=1 in the environment (fresh device buffers hold NaN / -1: a read of unwritten memory
shows in the results).  A launch may give up on a GPU that is shared; the step is then redone per step: its accuracy is held all
the same, and its form assertion is reported as an expected failure naming the give-up -- the last test counts them: the form
assertions of nine in ten fused cases must have held.  Measured ratios: profiles/r11_train_form_noise.txt."""
import pytest

from tests import grad_noise_cases as gn
from tests import train_form_cases as tf

pytestmark = pytest.mark.gpu

PARAMS = [(fc, path) for fc in tf.ALL for path in ('fused', 'stepwise')]       # (a case's two paths side by side: they share its oracles)
_FORM_HELD = {}                 # fused case -> did its form assertions hold (False: a give-up)


@pytest.mark.parametrize('fc,path', PARAMS, ids=['%s-%s' % (fc[0][0], path) for fc, path in PARAMS])
def test_step_within_float64_noise_bounds_in_the_predicted_form(fc, path):
    case = fc[0]
    name = case[0]
    cfg, w, inputs, batch, o64, o32 = tf.oracles(fc)
    e64, e32 = tf.eval_losses(fc)
    seen = {}

    def probe(eng):             # behind the mode-2 step: its statistics, then the mask-free evaluation and its statistics
        seen['cus'] = eng.stat('cus')
        seen['step'] = (eng.stat('train_persistent_launches'), eng.stat('train_give_ups'))
        seen['eval_loss'] = eng.train_step(*batch[:5], masks=None, mode=0)[0]
        seen['eval'] = (eng.stat('train_persistent_launches'), eng.stat('train_give_ups'))

    got = gn.device(case, w, batch, path, 0, probe)
    r = gn.ratios(got, o32, o64)
    form = tf.form(fc, cus=seen['cus'], persistent=path == 'fused')
    forward = sum(ln['persistent'] for ln in form['launches'] if ln['kind'] in ('rec', 'cell'))
    bounded = {k: v for k, v in r.items() if k not in gn.ZERO_GRADIENTS}
    k_rms, k_max = max(bounded, key=lambda k: bounded[k][0]), max(bounded, key=lambda k: bounded[k][1])
    eval_ratio = tf.scalar_ratio(seen['eval_loss'], e32, e64)
    print('train_form_noise %-14s %-8s rms_ratio %7.3f %-10s max_ratio %7.3f %-10s eval_loss_ratio %6.3f launches %2d predicted %2d '
          'eval_launches %d predicted %d give_ups %d cus %d' % (name, path, bounded[k_rms][0], k_rms, bounded[k_max][1], k_max, eval_ratio,
                                                               seen['step'][0], form['count'], seen['eval'][0], forward, seen['eval'][1], seen['cus']))
    # 1. accuracy (also of a step that was redone after a give-up)
    bad = {k: v for k, v in bounded.items() if v[0] > gn.C_RMS or v[1] > gn.C_MAX}
    assert not bad, (path, bad)
    for k in gn.ZERO_GRADIENTS:
        if k in o64[2]:
            assert gn.within_old_bound(got[2][k], o64[2][k], o64[1]), (path, k)
    # 4. the mask-free evaluation's loss (no regulariser in mode 0) in the same unit
    assert eval_ratio <= gn.C_MAX, (path, seen['eval_loss'], e64, e32)
    # 2. / 3. the form
    if path == 'stepwise':
        assert seen['step'] == (0, 0) and seen['eval'] == (0, 0)
        return
    if seen['eval'][1]:
        _FORM_HELD[name] = False
        pytest.xfail('%s: a persistent launch gave up (%d step(s) redone per step; is the GPU shared?): launches %d, predicted %d'
                     % (name, seen['eval'][1], seen['step'][0], form['count']))
    assert seen['step'] == (form['count'], 0), (name, seen, [(ln['kernel'], ln['NT'], ln['jobs']) for ln in form['launches'] if ln['persistent']])
    assert seen['eval'] == (forward, 0), (name, seen)
    assert form['count'] == fc[2] or seen['cus'] != 256, (name, form['count'])       # (the table's figure is for 256 CUs)
    _FORM_HELD[name] = True


def test_form_assertions_held_in_nine_of_ten_fused_cases():
    """Counts the fused cases of THIS run (above): a run in which more than one in ten gave up says nothing about the forms."""
    if not _FORM_HELD:          # (a selection without a fused case: nothing to count)
        return
    gave_up = sorted(k for k, ok in _FORM_HELD.items() if not ok)
    assert len(gave_up) <= len(_FORM_HELD) / 10, gave_up
