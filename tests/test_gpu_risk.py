"""Minimum-risk training on the device: the head alone (casv_debug_risk_rows) against its float64 definition -- the coefficients
given the device's own logp within tests/risk_cases.py's coefficient bound, the loss and dlogits within its noise bound --, the
whole mode-2 step against the oracle run twice (tests/risk_cases.step_reference) within tests/grad_noise_cases.py's constants, the
deterministic repeat, the argument errors and train(risk_samples=...)."""
import glob
import os

import numpy as np
import pytest

from tests import grad_noise_cases as gn
from tests import risk_cases as rc

pytestmark = pytest.mark.gpu

PADS = (0.0, float('nan'), 1e30)
# The whole step's constants: tests/grad_noise_cases.py's own.  Measured with alpha = rc.STEP_ALPHA (profiles/risk_noise.txt).
C_RMS, C_MAX = gn.C_RMS, gn.C_MAX


@pytest.fixture(scope='module')
def engine():
    from cor_asv_ann_amd.engine import HipEngine
    eng = HipEngine(1, 32, 40)
    yield eng
    eng.close()


# ---- the head alone ----
def head_figures(engine, case):
    """Per padding value: (coefficient error / its bound, q error / its bound, loss error / noise unit, dlogits error / noise
    unit, outputs) of the device head on a case.  The coefficient reference is head(float64) fed the device's own float32 logp."""
    (x, target, weight, cost, alpha, _), f64, f32 = rc.reference(case)
    V, N, G, U = case
    cb = rc.coef_bound(cost, alpha, N)
    unit = rc.bounds(f32, f64, c=1.0, coef_floor=cb)
    out = {}
    for pad in PADS:
        logp = engine.debug_score_rows(x.reshape(-1, V), target.reshape(-1), pad_value=pad)[0].reshape(target.shape)
        _, _, q_ref, c_ref = rc.head(x, target, weight, cost, alpha, N, np.float64, logp=logp)
        loss, q, coef, d = engine.debug_risk_rows(x, target, weight, cost, N, alpha, pad_value=pad)
        err = rc.errors((loss, d), f64)
        c_err = rc.coef_error(coef, c_ref)
        out[pad] = (c_err / cb if cb else c_err, float(np.abs(q - q_ref).max()) / (cb if cb else 1.0),
                    err[0] / unit[0], err[1] / unit[1], (loss, q, coef, d))
    return out


@pytest.mark.parametrize('case', rc.HEAD_CASES, ids=lambda c: 'V%d_N%d_G%d_U%d' % c)
def test_head_within_its_bounds(engine, case):
    (x, target, weight, cost, alpha, kinds), f64, f32 = rc.reference(case)
    V, N, G, U = case
    for pad, (c_ratio, q_ratio, loss_ratio, d_ratio, (loss, q, coef, d)) in head_figures(engine, case).items():
        print('V%d N%d G%d U%d pad %s: coef %.3g and q %.3g of the coefficient bound, loss %.3f and dlogits %.3f noise units'
              % (case + (pad, c_ratio, q_ratio, loss_ratio, d_ratio)))
        assert c_ratio <= 1.0 and q_ratio <= 1.0, (pad, c_ratio, q_ratio)
        assert loss_ratio <= rc.C and d_ratio <= rc.C, (pad, loss_ratio, d_ratio)
        # rows of zero kind are exactly zero; so is all of N = 1
        zero = (target < 0) | (weight == 0) | (cost < 0)[:, None]
        assert not d[zero].any(), pad
        assert not q[cost < 0].any() and not coef[cost < 0].any(), pad
        if N == 1:
            assert not d.any() and not coef.any() and np.all(q[cost >= 0] == 1.0), pad
            members = cost[cost >= 0].astype(np.float64)      # (the mean cost: one rounding per product and per add, in double)
            mean = float(members.sum()) / max(len(members), 1)
            assert abs(loss - mean) <= 2 * (G + 1) * 2.0 ** -53 * mean, (pad, loss, mean)


@pytest.mark.parametrize('case', [c for c in rc.HEAD_CASES if c[2] == 3 and c[0] in (5, 65)] + [(65, 3, 4, 7), (96, 64, 2, 7)],
                         ids=lambda c: 'V%d_N%d_G%d_U%d' % c)
def test_a_group_has_the_same_bits_alone_and_in_a_larger_call(engine, case):
    """q of a group launched alone = q of the same group as any group of the larger call, bit for bit; so is coef x G where the
    number of groups with a member is a power of two in both calls (inv is then exact, and so is the product: a float32 times 1/3
    times 3 is not) -- the cases with G = 4 and 2, whose groups all have members."""
    V, N, G, U = case
    x, target, weight, cost, alpha, kinds = rc.build(case)
    if G in (2, 4):
        cost = np.where(cost < 0, np.float32(0.5), cost).astype(np.float32)
    _, q_all, coef_all, _ = engine.debug_risk_rows(x, target, weight, cost, N, alpha, pad_value=float('nan'))
    for g in range(G):
        rows = slice(g * N, (g + 1) * N)
        _, q, coef, _ = engine.debug_risk_rows(x[rows], target[rows], weight[rows], cost[rows], N, alpha, pad_value=float('nan'))
        assert q.tobytes() == q_all[rows].tobytes(), g
        if G in (2, 4):
            assert coef.tobytes() == (coef_all[rows] * np.float32(G)).tobytes(), g


# ---- the whole step ----
def _device_risk(case, w, batch, N, cost, alpha, path, deterministic, steps=0):
    """(loss, norm, grads) of one mode-2 risk step; steps > 0: that many mode-1 steps instead, returns (weights, m, v, losses)."""
    from cor_asv_ann_amd.engine import HipEngine
    name, d, W, V, B, L, es, with_masks, flags, A, frozen = case
    sidx, val, d_in, d_out, wts, masks = batch
    eng = HipEngine(d, W, V, **flags)
    try:
        eng.set_weights(w)
        eng.set_option('persistent', -1 if path == 'fused' else 0)
        eng.set_option('fused_backward', 1 if path == 'fused' else 0)
        eng.set_option('deterministic', deterministic)
        eng.train_begin(frozen=frozen)
        if steps:
            losses = [eng.train_step_risk(sidx, val, d_in, d_out, wts, cost, N, alpha, masks, mode=1)[0] for _ in range(steps)]
            m, v, step = eng.train_state()
            assert step == steps
            out = (eng.train_weights(), m, v, losses)
        else:
            loss, norm, q, risk = eng.train_step_risk(sidx, val, d_in, d_out, wts, cost, N, alpha, masks, mode=2, details=True)
            assert q.shape == (B,) and risk.shape == (B // N,)
            for g in range(B // N):
                members = cost[g * N:(g + 1) * N] >= 0
                assert abs(q[g * N:(g + 1) * N][members].sum() - 1.0) < 1e-12 and not q[g * N:(g + 1) * N][~members].any()
            grads = {k: g for k, g in eng.train_gradients().items() if not (frozen and k.startswith(tuple(frozen)))}
            out = (float(loss), float(norm), grads)
        eng.train_end()
        return out
    finally:
        eng.close()


def step_ratios(name):
    """{(path, det): gn.ratios of the device's risk step} on a whole-step case, against the oracle in float32 and float64."""
    case, cfg, w, inputs, batch, N, cost = rc.step_inputs(name)
    o64, p64 = rc.step_reference(cfg, w, inputs, N, cost, rc.STEP_ALPHA, np.float64)
    o32, _ = rc.step_reference(cfg, w, inputs, N, cost, rc.STEP_ALPHA, np.float32)
    assert 1e-6 < p64[0] and p64[1] < 1 - 1e-6, p64
    out = {}
    for path, det in (('fused', 0), ('stepwise', 0), ('stepwise', 1)):
        got = _device_risk(case, w, batch, N, cost, rc.STEP_ALPHA, path, det)
        out[(path, det)] = (gn.ratios(got, o32, o64), got, o64)
    return out


@pytest.mark.parametrize('name', sorted(rc.STEP_CASES))
def test_risk_step_within_float64_noise_bounds(name):
    for (path, det), (r, got, o64) in step_ratios(name).items():
        seen = {k: v for k, v in r.items() if k not in gn.ZERO_GRADIENTS}
        print('%s %s det %d alpha %g: largest rms ratio %.2f, largest max ratio %.2f' % (
            name, path, det, rc.STEP_ALPHA, max(v[0] for v in seen.values()), max(v[1] for v in seen.values())))
        bad = {k: v for k, v in seen.items() if v[0] > C_RMS or v[1] > C_MAX}
        assert not bad, (path, det, bad)
        for k in gn.ZERO_GRADIENTS:
            if k in o64[2]:
                assert gn.within_old_bound(got[2][k], o64[2][k], o64[1]), (path, det, k)


def test_deterministic_risk_steps_repeat_bit_for_bit():
    case, cfg, w, inputs, batch, N, cost = rc.step_inputs('d2_w32_b4_m')
    a = _device_risk(case, w, batch, N, cost, rc.STEP_ALPHA, 'stepwise', 1, steps=2)
    b = _device_risk(case, w, batch, N, cost, rc.STEP_ALPHA, 'stepwise', 1, steps=2)
    assert a[3] == b[3] and all(np.isfinite(a[3]))
    for x, y in zip(a[:3], b[:3]):
        assert set(x) == set(y)
        for k in x:
            assert np.array_equal(x[k], y[k]), k
    assert any(not np.array_equal(a[0][k], w[k]) for k in w)          # (the steps moved the weights)


def test_bad_risk_arguments_are_refused_and_leave_the_session_untouched():
    from cor_asv_ann_amd._native import NativeError
    from cor_asv_ann_amd.engine import HipEngine
    case, cfg, w, inputs, batch, N, cost = rc.step_inputs('d2_w32_b4_m')
    sidx, val, d_in, d_out, wts, masks = batch
    eng = HipEngine(case[1], case[2], case[3])
    try:
        eng.set_weights(w)
        eng.set_option('deterministic', 1)
        eng.train_begin()
        eng.train_step_risk(sidx, val, d_in, d_out, wts, cost, N, rc.STEP_ALPHA, masks, mode=1)
        before = (eng.train_state(), eng.train_gradients())

        def with_cost(i, value):
            c = cost.copy()
            c[i] = value
            return c
        bad = {'mode 0': dict(mode=0), 'mode 3': dict(mode=3), 'N = 0': dict(n=0), 'N = 65': dict(n=65), 'N = 3 of B = 4': dict(n=3),
               'no cost': dict(cost=None), 'NaN cost': dict(cost=with_cost(1, np.nan)), 'infinite cost': dict(cost=with_cost(2, np.inf)),
               'cost minus infinity': dict(cost=with_cost(0, -np.inf)), 'alpha NaN': dict(alpha=float('nan')),
               'alpha infinite': dict(alpha=float('inf')), 'alpha 0': dict(alpha=0.0), 'alpha negative': dict(alpha=-1.0)}
        for what, change in bad.items():
            kw = dict(cost=cost, n=N, alpha=rc.STEP_ALPHA, mode=1)
            kw.update(change)
            for mode in ((kw['mode'],) if 'mode' in change else (1, 2)):
                with pytest.raises(NativeError) as err:
                    eng.train_step_risk(sidx, val, d_in, d_out, wts, kw['cost'], kw['n'], kw['alpha'], masks, mode=mode)
                assert err.value.code == -1, (what, mode, str(err.value))        # CASV_ERR_ARG
            (m, v, step), grads = eng.train_state(), eng.train_gradients()
            assert step == before[0][2] == 1, what
            for k in grads:
                assert np.array_equal(grads[k], before[1][k]), (what, k)
            for k in m:
                assert np.array_equal(m[k], before[0][0][k]) and np.array_equal(v[k], before[0][1][k]), (what, k)
        loss, _ = eng.train_step_risk(sidx, val, d_in, d_out, wts, cost, N, rc.STEP_ALPHA, masks, mode=2)      # (the session still works)
        assert np.isfinite(loss)
        eng.train_end()
    finally:
        eng.close()


# ---- the loop ----
def _model(epochs=2):
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence
    s2s = Sequence2Sequence(progbars=False)
    s2s.depth, s2s.width, s2s.batch_size, s2s.epochs = 1, 32, 32, epochs
    s2s.seed, s2s.deterministic, s2s.checkpoint_training_state = 11, True, True
    s2s.configure()
    return s2s


def _checkpoints(epoch):
    found = sorted(glob.glob('model.ckpt.weights-%02d-*.h5' % epoch))
    assert len(found) == 1, found
    return found[0]


def test_train_with_risk_samples_checkpoints_and_resumes(tmp_path, monkeypatch):
    """Two epochs with risk_samples = 4; resumed from the first epoch's checkpoint the second epoch repeats bit for bit (the
    candidates' seed and the lines' running numbers are the file's and the epoch's); another risk_alpha is refused; and a run
    without risk_samples writes a training state with the keys it always had."""
    from cor_asv_ann_amd import keras_h5
    from cor_asv_ann_amd.synthetic import make_lines
    lines, _ = make_lines(320, 9, 5, voc_size=24)
    corpus = str(tmp_path / 'train.tsv')
    with open(corpus, 'w') as f:
        f.write(''.join('%s\t%s\n' % (l[:-1], l[:-1]) for l in lines))
    (tmp_path / 'risk').mkdir()
    monkeypatch.chdir(tmp_path / 'risk')
    whole = _model()
    whole.train([corpus], risk_samples=4, risk_alpha=0.5)
    assert len(whole.history) == 2 and all(np.isfinite(h['loss']) and np.isfinite(h['val_loss']) for h in whole.history), whole.history
    assert all(0.0 <= h['loss'] for h in whole.history)               # (an expected normalised edit distance)
    first = os.path.abspath(_checkpoints(1))
    state = keras_h5.read_training_state(first)
    assert state['risk']['samples'] == 4 and state['risk']['alpha'] == 0.5 and state['risk']['own_proposal'] is True
    (tmp_path / 'resumed').mkdir()
    monkeypatch.chdir(tmp_path / 'resumed')
    again = _model()
    with pytest.raises(ValueError, match='risk alpha differs'):
        again.train([corpus], resume=first, risk_samples=4, risk_alpha=0.25)
    with pytest.raises(ValueError, match='risk_samples'):
        again.train([corpus], resume=first)
    again = _model()
    again.train([corpus], resume=first, risk_samples=4, risk_alpha=0.5)
    assert again.history == whole.history
    for k, v in whole._weights.items():
        assert np.array_equal(again._weights[k], v), k
    # a plain run: no new keys in its state, and no resuming it as a minimum-risk run
    (tmp_path / 'plain').mkdir()
    monkeypatch.chdir(tmp_path / 'plain')
    plain = _model(epochs=1)
    plain.train([corpus], risk_samples=0)
    ckpt = os.path.abspath(_checkpoints(1))
    assert 'risk' not in keras_h5.read_training_state(ckpt)
    assert b'risk' not in open(ckpt, 'rb').read()
    with pytest.raises(ValueError, match='without risk_samples'):
        _model().train([corpus], resume=ckpt, risk_samples=4)
