"""Soft targets on the device: the loss head alone (casv_debug_soft_ce_rows) against its float64 definition within the noise bound
of tests/soft_target_cases.py, the whole mode-2 step against the float64 oracle within tests/grad_noise_cases.py's constants, the
one-hot lists against the hard step bit for bit, the deterministic repeat, the argument errors and train(teacher=...)."""
import numpy as np
import pytest

from oracle.train import forward_backward
from tests import grad_noise_cases as gn
from tests import soft_target_cases as sc

pytestmark = pytest.mark.gpu

STEP_CASES = [c for c in gn.CASES if c[0] in ('d1_w32_b4', 'd2_w32_b4_m', 'd3_w64_b8_m', 'deep', 'confusion', 'frozen')]


@pytest.fixture(scope='module')
def engine():
    from cor_asv_ann_amd.engine import HipEngine
    eng = HipEngine(1, 32, 40)
    yield eng
    eng.close()


# ---- the head alone ----
@pytest.mark.parametrize('case', sc.HEAD_CASES, ids=lambda c: 'V%d_K%d_R%d' % c)
def test_head_within_the_noise_bound(engine, case):
    """Loss and dlogits within C x the float32 head's own error of the float64 head; the padding columns hold NaN or 1e30 on the
    way in and come back as zeros (the entry checks); plain and ordered sums; without gradients the loss alone."""
    (x, idx, q, w, inv_count, _), f64, f32 = sc.reference(case)
    bound = sc.bounds(f32, f64)
    worst = 0.0
    for pad in (float('nan'), 1e30):
        for ordered in (False, True):
            loss, d = engine.debug_soft_ce_rows(x, idx, q, w, inv_count, pad_value=pad, want_grad=True, ordered=ordered)
            err = sc.errors((loss, d), f64)
            worst = max(worst, max(e / (b / sc.C) for e, b in zip(err, bound)))
            print('V%d K%d R%d pad %s ordered %d: loss error %.3g (bound %.3g), dlogits error %.3g (bound %.3g)'
                  % (case + (pad, ordered, err[0], bound[0], err[1], bound[1])))
            assert err[0] <= bound[0] and err[1] <= bound[1], (pad, ordered, err, bound)
            only, none = engine.debug_soft_ce_rows(x, idx, q, w, inv_count, pad_value=pad, want_grad=False, ordered=ordered)
            assert none is None and abs(only - f64[0]) <= bound[0], (pad, ordered, only, f64[0])
            if ordered:
                assert only == loss                     # (the ordered sum: the same bits with and without the gradient pass)
    print('V%d K%d R%d: largest ratio %.3f' % (case + (worst,)))


def test_head_rows_of_zero_kind_are_zero(engine):
    """All slots empty, or weight 0: no loss, a zero gradient row (exactly)."""
    case = (65, 3, 8197)
    (x, idx, q, w, inv_count, kinds), _, _ = sc.reference(case)
    zero = np.array([k in ('all_empty', 'weight_0') for k in kinds])
    loss, d = engine.debug_soft_ce_rows(x[zero], idx[zero], q[zero], w[zero], inv_count, pad_value=float('nan'))
    assert loss == 0.0 and not d.any()


# ---- the whole step ----
def _soft_case(case):
    """The case of tests/grad_noise_cases.py with its target rows replaced by normalised K = 4 soft rows (the hard target and the
    float64 oracle's three likeliest other characters); the oracle's probabilities of all entries with q > 0 are inside
    (1e-6, 1 - 1e-6): the condition under which the oracle's backward (one factor per row) is the definition (one per entry)."""
    cfg, w, inputs, batch = gn.build(case)
    enc_in, dec_in, dec_out, wts, masks = inputs
    cast = lambda a: np.asarray(a, np.float64)
    m64 = None if masks is None else {'enc': [cast(a) for a in masks['enc']], 'dec': [cast(a) for a in masks['dec']], 'cell': cast(masks['cell'])}
    _, _, aux = forward_backward(cfg, {k: cast(v) for k, v in w.items()}, cast(enc_in), cast(dec_in), cast(dec_out), cast(wts), m64,
                                 want_grads=False, window_dtype=np.float32)
    dense, soft_idx, soft_q = sc.soften(dec_out, aux['probs'])
    p = aux['probs'][dense > 0]
    assert p.size and p.min() > 1e-6 and p.max() < 1 - 1e-6, (p.min(), p.max())
    assert np.allclose(dense.sum(axis=2)[np.asarray(dec_out).any(axis=2)], 1.0, atol=1e-6)
    sidx, val, d_in, _, wts_d, masks_d = batch
    return cfg, w, (enc_in, dec_in, dense, wts, masks), (sidx, val, d_in, soft_idx, soft_q, wts_d, masks_d)


def _device_soft(case, w, batch, path, deterministic, steps=0):
    """(loss, norm, grads) of one mode-2 soft step; steps > 0: that many mode-1 steps instead, returns (weights, m, v, losses)."""
    from cor_asv_ann_amd.engine import HipEngine
    name, d, W, V, B, L, es, with_masks, flags, A, frozen = case
    eng = HipEngine(d, W, V, **flags)
    try:
        eng.set_weights(w)
        eng.set_option('persistent', -1 if path == 'fused' else 0)
        eng.set_option('fused_backward', 1 if path == 'fused' else 0)
        eng.set_option('deterministic', deterministic)
        eng.train_begin(frozen=frozen)
        if steps:
            losses = [eng.train_step_soft(*batch, mode=1)[0] for _ in range(steps)]
            m, v, step = eng.train_state()
            assert step == steps
            out = (eng.train_weights(), m, v, losses)
        else:
            loss, norm = eng.train_step_soft(*batch, mode=2)
            grads = {k: g for k, g in eng.train_gradients().items() if not (frozen and k.startswith(tuple(frozen)))}
            out = (float(loss), float(norm), grads)
        eng.train_end()
        return out
    finally:
        eng.close()


@pytest.mark.parametrize('case', STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_soft_step_within_float64_noise_bounds(case):
    cfg, w, inputs, batch = _soft_case(case)
    frozen = case[10]
    o64, o32 = gn.oracle(cfg, w, inputs, np.float64, frozen), gn.oracle(cfg, w, inputs, np.float32, frozen)
    for path, det in (('fused', 0), ('stepwise', 0), ('stepwise', 1)):
        got = _device_soft(case, w, batch, path, det)
        r = gn.ratios(got, o32, o64)
        seen = {k: v for k, v in r.items() if k not in gn.ZERO_GRADIENTS}
        print('%s %s det %d: largest rms ratio %.2f, largest max ratio %.2f' % (
            case[0], path, det, max(v[0] for v in seen.values()), max(v[1] for v in seen.values())))
        bad = {k: v for k, v in seen.items() if v[0] > gn.C_RMS or v[1] > gn.C_MAX}
        assert not bad, (path, det, bad)
        for k in gn.ZERO_GRADIENTS:
            if k in o64[2]:
                assert gn.within_old_bound(got[2][k], o64[2][k], o64[1]), (path, det, k)


@pytest.mark.parametrize('name', ['d2_w32_b4_m', 'd3_w64_b8_m'])
def test_one_hot_lists_are_the_hard_step_bit_for_bit(name):
    """deterministic = 1: K = 1 lists (dec_out, 1.0) give the hard step's loss bits and its gradients."""
    case = [c for c in gn.CASES if c[0] == name][0]
    cfg, w, inputs, batch = gn.build(case)
    sidx, val, d_in, d_out, wts, masks = batch
    hard = gn.device(case, w, batch, 'stepwise', 1)
    soft_idx = d_out[:, :, None].astype(np.int32)
    soft_q = np.ones(soft_idx.shape, np.float32)
    soft = _device_soft(case, w, (sidx, val, d_in, soft_idx, soft_q, wts, masks), 'stepwise', 1)
    assert np.float64(soft[0]).tobytes() == np.float64(hard[0]).tobytes() and soft[1] == hard[1]
    assert set(soft[2]) == set(hard[2])
    for k in hard[2]:
        assert np.array_equal(soft[2][k], hard[2][k]), k
    # ... and with the slot anywhere among K = 3, beside empty slots
    wide_idx = np.full(d_out.shape + (3,), -1, np.int32)
    wide_idx[:, :, 1] = d_out
    wide = _device_soft(case, w, (sidx, val, d_in, wide_idx, np.full(wide_idx.shape, 1.0, np.float32), wts, masks), 'stepwise', 1)
    assert wide[0] == hard[0] and all(np.array_equal(wide[2][k], hard[2][k]) for k in hard[2])


def test_deterministic_soft_steps_repeat_bit_for_bit():
    case = [c for c in gn.CASES if c[0] == 'd2_w32_b4_m'][0]
    cfg, w, inputs, batch = _soft_case(case)
    a = _device_soft(case, w, batch, 'stepwise', 1, steps=3)
    b = _device_soft(case, w, batch, 'stepwise', 1, steps=3)
    assert a[3] == b[3] and all(np.isfinite(a[3]))
    for x, y in zip(a[:3], b[:3]):
        assert set(x) == set(y)
        for k in x:
            assert np.array_equal(x[k], y[k]), k
    assert any(not np.array_equal(a[0][k], w[k]) for k in w)          # (the steps moved the weights)


def test_bad_soft_targets_are_refused_and_leave_the_session_untouched():
    from cor_asv_ann_amd._native import NativeError
    from cor_asv_ann_amd.engine import HipEngine
    case = [c for c in gn.CASES if c[0] == 'd2_w32_b4_m'][0]
    cfg, w, inputs, batch = _soft_case(case)
    sidx, val, d_in, soft_idx, soft_q, wts, masks = batch
    V = case[3]
    eng = HipEngine(case[1], case[2], V)
    try:
        eng.set_weights(w)
        eng.set_option('deterministic', 1)
        eng.train_begin()
        eng.train_step_soft(*batch, mode=1)
        before = (eng.train_state(), eng.train_gradients())
        b, u = np.argwhere(soft_idx[:, :, 0] >= 0)[1]
        wide = min(V, 64) + 1
        bad = {'K = 0': (np.zeros(soft_idx.shape[:2] + (0,), np.int32), np.zeros(soft_idx.shape[:2] + (0,), np.float32)),
               'K above min(V, 64)': (np.full(soft_idx.shape[:2] + (wide,), -1, np.int32), np.zeros(soft_idx.shape[:2] + (wide,), np.float32))}
        bad['index below -1'] = _set(soft_idx, soft_q, b, u, 'i', 2, -2)
        bad['index V'] = _set(soft_idx, soft_q, b, u, 'i', 2, V)
        bad['negative mass'] = _set(soft_idx, soft_q, b, u, 'q', 1, -0.25)
        bad['NaN mass'] = _set(soft_idx, soft_q, b, u, 'q', 1, np.nan)
        bad['infinite mass'] = _set(soft_idx, soft_q, b, u, 'q', 3, np.inf)
        bad['repeated index'] = _set(soft_idx, soft_q, b, u, 'i', 3, soft_idx[b, u, 0])
        for what, (i, q) in bad.items():
            for mode in (0, 1, 2):
                with pytest.raises(NativeError) as err:
                    eng.train_step_soft(sidx, val, d_in, i, q, wts, masks, mode=mode)
                assert err.value.code == -1, (what, mode, str(err.value))        # CASV_ERR_ARG
            (m, v, step), grads = eng.train_state(), eng.train_gradients()
            assert step == before[0][2] == 1, what
            for k in grads:
                assert np.array_equal(grads[k], before[1][k]), (what, k)
            for k in m:
                assert np.array_equal(m[k], before[0][0][k]) and np.array_equal(v[k], before[0][1][k]), (what, k)
        # an empty slot's mass is ignored, whatever it holds
        i, q = _set(soft_idx, soft_q, b, u, 'i', 3, -1)
        q[b, u, 3] = np.nan
        loss, _ = eng.train_step_soft(sidx, val, d_in, i, q, wts, masks, mode=0)
        assert np.isfinite(loss)
        eng.train_end()
    finally:
        eng.close()


def _set(soft_idx, soft_q, b, u, which, k, value):
    i, q = soft_idx.copy(), soft_q.copy()
    (i if which == 'i' else q)[b, u, k] = value
    return i, q


# ---- the loop ----
def _student(tmp_path, sub, corpus, depth=1, epochs=2):
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence
    s2s = Sequence2Sequence(progbars=False)
    s2s.depth, s2s.width, s2s.batch_size, s2s.epochs = depth, 32, 32, epochs
    s2s.seed, s2s.deterministic = 11, True
    s2s.configure()
    return s2s


def test_train_with_a_teacher(tmp_path, monkeypatch):
    """alpha = 1: the distilled run IS the plain run (one-hot lists through the soft step), weights equal bit for bit; alpha = 0.5:
    the run completes with finite losses and other weights."""
    from cor_asv_ann_amd.synthetic import make_lines
    lines, _ = make_lines(320, 9, 5, voc_size=24)
    corpus = str(tmp_path / 'train.tsv')
    with open(corpus, 'w') as f:
        f.write(''.join('%s\t%s\n' % (l[:-1], l[:-1]) for l in lines))
    teacher = _student(tmp_path, 'teacher', corpus, depth=2)
    teacher.map_files([corpus])
    teacher.status = 2
    runs = {}
    for sub, kw in (('plain', {}), ('alpha1', dict(teacher=teacher, distill_alpha=1.0)), ('alpha05', dict(teacher=teacher, distill_alpha=0.5))):
        (tmp_path / sub).mkdir()
        monkeypatch.chdir(tmp_path / sub)
        s2s = _student(tmp_path, sub, corpus)
        s2s.train([corpus], **kw)
        assert len(s2s.history) == 2 and all(np.isfinite(h['loss']) and np.isfinite(h['val_loss']) for h in s2s.history), (sub, s2s.history)
        runs[sub] = s2s
    assert runs['alpha1'].history == runs['plain'].history
    for k, v in runs['plain']._weights.items():
        assert np.array_equal(runs['alpha1']._weights[k], v), k
    assert any(not np.array_equal(runs['alpha05']._weights[k], v) for k, v in runs['plain']._weights.items())
    assert runs['alpha05'].history[0]['loss'] != runs['plain'].history[0]['loss']
