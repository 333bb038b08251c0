"""The decode path against float64, in units of the fp32 oracle's own rounding noise (tests/decode_noise_cases.py): the encoder
(persistent and per-step chain, split arithmetic at a small and a large size, depth 1, width 100, the optional topologies, a
confusion-network input, 100-character lines) and teacher-forced decoder / LM steps (casv_decoder_step_lm) under arithmetic 0 and 2
at row counts that reach every tile shape, ragged tails and the page shape's partial round.  tests/test_decode_noise_bounds.py shows
without a GPU that the bounds see one-row mistakes."""
import numpy as np
import pytest

from tests import decode_noise_cases as dn

pytestmark = pytest.mark.gpu


def _check(got, o32, o64, where):
    assert not dn.nan_mismatch(got, o32), (where, dn.nan_mismatch(got, o32))
    r = dn.ratios(got, o32, o64)
    bad = {k: v for k, v in r.items() if v[0] > dn.C_RMS or v[1] > dn.C_MAX}
    assert not bad, (where, bad)


@pytest.mark.parametrize('case', dn.ENC_CASES, ids=[c[0] for c in dn.ENC_CASES])
def test_encoder_within_float64_noise_bounds(case):
    cfg, w, x, inputs = dn.build_encoder(case)
    o32, o64 = dn.oracle_encoder(cfg, w, x, np.float32), dn.oracle_encoder(cfg, w, x, np.float64)
    _check(dn.device_encoder(case, w, inputs), o32, o64, case[0])


@pytest.mark.parametrize('case', dn.STEP_CASES, ids=[c[0] for c in dn.STEP_CASES])
def test_decoder_steps_within_float64_noise_bounds(case):
    cfg, w, (line, enc, states, a, p_in) = dn.build_step(case)
    engs = {ar: dn.step_engine(cfg, w, enc, ar) for ar in (0, 2)}
    try:
        for s in range(case[7]):
            o32 = dn.oracle_step(cfg, w, line, enc, states, a, p_in, np.float32)
            o64 = dn.oracle_step(cfg, w, line, enc, states, a, p_in, np.float64)
            for ar, eng in engs.items():
                _check(dn.device_step(eng, line, states, a, p_in), o32, o64, (s, ar))
            states, a, p_in = dn.next_inputs(cfg, o32)
    finally:
        for eng in engs.values():
            eng.close()
