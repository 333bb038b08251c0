"""The train step's loss, norm and every gradient against float64, in units of the fp32 oracle's own rounding noise
(tests/grad_noise_cases.py): the shapes of tests/test_gpu_train.py, one case per optional topology, a confusion-network input,
frozen layers and a mid-size batch whose weight gradients take the split and ordered split forms -- fused and stepwise recurrences,
deterministic off and on.  tests/test_grad_noise_bounds.py shows without a GPU that the bounds see a one-step mistake."""
import numpy as np
import pytest

from tests import grad_noise_cases as gn
from tests.tn_reference import plan

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case', gn.ALL, ids=[c[0] for c in gn.ALL])
def test_step_within_float64_noise_bounds(case):
    cfg, w, inputs, batch = gn.build(case)
    frozen = case[10]
    o64, o32 = gn.oracle(cfg, w, inputs, np.float64, frozen), gn.oracle(cfg, w, inputs, np.float32, frozen)
    if case is gn.MID:          # the encoder's weight gradients: split kernel, atomic and ordered (plan mirror, 256 CUs)
        W, B, T = case[2], case[4], batch[0].shape[1]
        assert plan(4 * W, W, B * T, 2, False)[0] == 1 and plan(4 * W, W, B * T, 2, True)[0] == 1, T
    for path in ('fused', 'stepwise'):
        for det in (0, 1):
            got = gn.device(case, w, batch, path, det)
            r = gn.ratios(got, o32, o64)
            bad = {k: v for k, v in r.items() if k not in gn.ZERO_GRADIENTS and (v[0] > gn.C_RMS or v[1] > gn.C_MAX)}
            assert not bad, (path, det, bad)
            for k in gn.ZERO_GRADIENTS:
                if k in o64[2]:
                    assert gn.within_old_bound(got[2][k], o64[2][k], o64[1]), (path, det, k)
