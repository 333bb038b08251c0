"""Without a GPU: the noise bounds of tests/test_gpu_decode_noise.py would see a decode step or an encoder that gets one row, one
unit or one function range wrong.  Each mutation of the float64 oracle (tests/decode_noise_cases.py: step_mutations,
encoder_mutations) moves a probability, a state, an alignment or an encoder output at least 10x past C_RMS x noise_rms or
C_MAX x noise_max."""
import numpy as np
import pytest

from tests import decode_noise_cases as dn

STEP = dn.STEP_CASES[0]
ENC = [c for c in dn.ENC_CASES if c[0] in ('persist_d2_w256_b64', 'd1_w256_b48')]


def test_step_mutations_exceed_the_noise_bound():
    cfg, w, inputs = dn.build_step(STEP)
    o32 = dn.oracle_step(cfg, w, *inputs, np.float32)
    o64 = dn.oracle_step(cfg, w, *inputs, np.float64)
    for name, got in dn.step_mutations(cfg, w, inputs, o64).items():
        ex = dn.excess(dn.ratios(got, o32, o64))
        assert ex >= 10, (name, ex)


@pytest.mark.parametrize('case', ENC, ids=[c[0] for c in ENC])
def test_encoder_mutations_exceed_the_noise_bound(case):
    cfg, w, x, _ = dn.build_encoder(case)
    o32, o64 = dn.oracle_encoder(cfg, w, x, np.float32), dn.oracle_encoder(cfg, w, x, np.float64)
    for name, got in dn.encoder_mutations(cfg, w, x).items():
        ex = dn.excess(dn.ratios(got, o32, o64))
        assert ex >= 10, (name, ex)
