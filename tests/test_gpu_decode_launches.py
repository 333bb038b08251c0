"""The launch list of one decoder step (csrc/decode.hip, launch_step), counted through the profile (which bypasses the step
graph): per step of a greedy decode, of a beam search and of the explicit decoder step, at depths 1, 2 and 3.

A decode call is made twice, with 3 and with 6 steps, each on a fresh encoding: the difference of the two counts is three steps'
launches -- the encoder pass and the per-call set-up cancel.  With at most 16 steps the search is one chunk and runs exactly
`steps` iterations whatever the lines do.  "lstm" = lstm_gemm + lstm_gemm_small (the tile shape is the launcher's business).

    per step                         lstm  gemm  attention  softmax  beam  persist
    greedy, depth 1                    1     2       1         1      0      0       query | top cell | projection
    greedy, depth D >= 2               D     1       1         1      0      0       layer 1 + query | ... | top cell | projection
    beam, depth D (lm_predict or not)  D     1       1         0      1      0       the query rides in the projection's launch

The LM cell and the LM projection of lm_predict are further jobs of the top cell's and the projection's launches, not launches."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import ModelConfig, make_weights

W, V, B, T = 64, 48, 5, 6
CLASSES = ('lstm_gemm', 'lstm_gemm_small', 'gemm', 'attention', 'softmax', 'beam', 'persist')
KEYS = ('lstm', 'gemm', 'attention', 'softmax', 'beam', 'persist')


def _lines():
    """B ragged lines on T positions (lengths 6, 1, 4, 3, 5), the end-of-line character (index 1) last."""
    rng = np.random.default_rng(3)
    idx = np.full((B, T, 2), -1, np.int32)
    val = np.zeros((B, T, 2), np.float32)
    for j, n in enumerate((6, 1, 4, 3, 5)):
        idx[j, :n - 1, 0] = rng.integers(2, V, n - 1)
        val[j, :n - 1, 0] = 0.9
        idx[j, n - 1, 0], val[j, n - 1, 0] = 1, 1.0
    return idx, val


def _counts(eng):
    c = {k: eng.profile_read(k)['launches'] for k in CLASSES}
    c['lstm'] = c.pop('lstm_gemm') + c.pop('lstm_gemm_small')
    return tuple(c[k] for k in KEYS)


def _profiled(eng, call, encoded_ahead=False):
    """Launch counts of `call` on a fresh encoding; encoded_ahead: the chain arithmetic's encoder pass runs before the profile is
    switched on, so that the counts are the call's own."""
    eng.encode(*_lines())
    if encoded_ahead:
        eng.encoder_outputs()
    eng.profile(1)
    call()
    got = _counts(eng)
    eng.profile(0)
    return got


def _per_three_steps(eng, call):
    a, b = (_profiled(eng, lambda: call(steps)) for steps in (3, 6))
    print(a, b)
    return tuple(y - x for x, y in zip(a, b))


@pytest.fixture(scope='module', params=[1, 2, 3])
def engine(request):
    from cor_asv_ann_amd.engine import HipEngine
    cfg = ModelConfig(depth=request.param, width=W, voc_size=V)
    eng = HipEngine(cfg.depth, cfg.width, cfg.voc_size)
    eng.set_weights(make_weights(cfg, emb_scale=8.0))
    eng.set_option('persistent', 0)
    yield eng
    eng.close()


def _step(D, **kw):
    """KEYS of one step: lstm, gemm, attention, softmax, beam, persist."""
    return (D, 2 if D == 1 and 'softmax' in kw else 1, 1, kw.get('softmax', 0), kw.get('beam', 0), 0)


@pytest.mark.parametrize('mode', [0, 1])
def test_greedy_step(engine, mode):
    D = engine.depth
    got = _per_three_steps(engine, lambda steps: engine.decode_greedy(mode=mode, steps=steps))
    assert got == tuple(3 * n for n in _step(D, softmax=1))


@pytest.mark.parametrize('lm_predict', [0, 1])
def test_beam_step(engine, lm_predict):
    D = engine.depth
    engine.set_option('lm_predict', lm_predict)
    try:
        got = _per_three_steps(engine, lambda steps: engine.decode_beam(batch_size=4, steps=steps))
    finally:
        engine.set_option('lm_predict', 0)
    assert got == tuple(3 * n for n in _step(D, beam=1))


def test_persistent_greedy_is_one_launch_whatever_the_steps(engine):
    """(The chain arithmetic's encoder pass, a persistent launch of its own under this option, runs ahead of the profile.)"""
    engine.set_option('persistent', 1)
    try:
        counts = [_profiled(engine, lambda: engine.decode_greedy(mode=0, steps=steps), encoded_ahead=True) for steps in (3, 6)]
    finally:
        engine.set_option('persistent', 0)
    print(counts)
    assert counts[0] == counts[1] == (0, 0, 0, 0, 0, 1)


@pytest.mark.parametrize('lm', [False, True])
def test_explicit_decoder_step(engine, lm):
    """One step, nothing to take a difference of: the chain arithmetic's encoding is on the device before the profile is on."""
    D = engine.depth
    engine.encode(*_lines())
    enc, states = engine.encoder_outputs()
    p_in = np.zeros((B, V), np.float32)
    p_in[:, 2] = 1.0
    args = (np.arange(B, dtype=np.int32), p_in, states, np.zeros((B, T), np.float32))
    engine.profile(1)
    (engine.decoder_step_lm if lm else engine.decoder_step)(*args)
    got = _counts(engine)
    engine.profile(0)
    print(got)
    assert got == _step(D, softmax=1)
