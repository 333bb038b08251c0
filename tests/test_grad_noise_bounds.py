"""Without a GPU: the noise bounds of tests/test_gpu_grad_noise.py would see a train step that gets one step of one line wrong.
Each mutation of a case's inputs (tests/grad_noise_cases.py, mutations) moves the float64 oracle's loss, norm or a gradient at least
10x past C_RMS x noise_rms or C_MAX x noise_max."""
import numpy as np
import pytest

from tests import grad_noise_cases as gn


@pytest.mark.parametrize('case', gn.CASES, ids=[c[0] for c in gn.CASES])
def test_one_step_mutations_exceed_the_noise_bound(case):
    cfg, w, inputs, _ = gn.build(case)
    o64, o32 = gn.oracle(cfg, w, inputs, np.float64, case[10]), gn.oracle(cfg, w, inputs, np.float32, case[10])
    for name, got in gn.mutations(cfg, w, inputs, case[10]).items():
        excess = gn.excess(gn.ratios(got, o32, o64))
        assert excess >= 10, (name, excess)
