"""Without a GPU: the case table of tests/update_cases.py reaches what it claims, and the bounds of tests/test_gpu_update.py have
teeth -- a float32 numpy run of the restated update passes them, and each of eight mistakes an update could make exceeds one of
them at least 10x on at least one case (ratios in profiles/r10_update_error.txt).  Also: how far oracle.train.adam_step is from
the restatement."""
import functools

import numpy as np
import pytest

from oracle.train import adam_step
from tests import grad_noise_cases as gn
from tests import update_cases as uc


@functools.lru_cache(maxsize=None)
def _oracles(name):
    case = uc.BY_NAME[name]
    cfg, w, inputs, _ = gn.build(case)
    return w, gn.oracle(cfg, w, inputs, np.float32, ()), gn.oracle(cfg, w, inputs, np.float64, ())


def _norm(o, names):
    return float(np.sqrt(uc.sumsq(o[2], names)))


@pytest.mark.parametrize('case', uc.CASES, ids=[c[0] for c in uc.CASES])
def test_case_table_reaches_what_it_claims(case):
    names = uc.trained(uc.tensor_names(case), case[10])
    assert len(names) == uc.TENSORS[case[0]]
    assert (len(names) > uc.MULTI_MAX) == (case[0] in uc.SECOND_LIST)
    if case[10]:
        assert len(names) < len(uc.tensor_names(case))
    # clipped / unclipped membership of the hyper-parameter sets: the fp32 and the float64 oracle's norms lie on the same side
    w, o32, o64 = _oracles(case[0])
    for hname, hyper in uc.HYPERS.items():
        sides = [uc.scale_of(hyper, _norm(o, names))[1] for o in (o32, o64)]
        assert sides == [uc.CLIPS[hname]] * 2, (hname, _norm(o32, names), _norm(o64, names))


MUTATED_CASES = [uc.BY_NAME[k] for k in ('d2_w32', 'frozen', 'd8_w32', 'd5_deep_bridge')]


def _setups(case, full):
    """(w, m, v, g, names, step, hyper) of the float32 runs of a case: the fp32 oracle's gradients, every hyper-parameter set, seeded
    moments at every step count and zero moments at step 0 (not full: the two clipping sets, counts 1 and 999)."""
    w, o32, _ = _oracles(case[0])
    g = {k: np.asarray(a, np.float32) for k, a in o32[2].items()}
    names = uc.trained(list(w), case[10])
    zeros = {k: np.zeros_like(w[k]) for k in names}
    for hname, hyper in uc.HYPERS.items():
        if not full and hname not in ('default', 'other'):
            continue
        yield w, zeros, zeros, g, names, 0, hyper
        for i, step in enumerate(uc.STEPS if full else (1, 999)):
            m, v = uc.seeded_moments({k: w[k].shape for k in names}, 100 + i)
            yield w, m, v, g, names, step, hyper


def _worst(case, mutation):
    worst = {'norm': 0.0, 'm': 0.0, 'v': 0.0, 'w': 0.0}
    for w, m, v, g, names, step, hyper in _setups(case, mutation is None):
        gnorm, w2, m2, v2 = uc.simulate(w, m, v, g, step, hyper, names, mutation)
        r = uc.check((w, m, v), (w2, m2, v2), g, gnorm, step, hyper, names)
        if mutation is None:
            assert r['moved'] == 0
        for q in worst:
            worst[q] = max(worst[q], r[q])
    return worst


@pytest.mark.parametrize('case', uc.CASES, ids=[c[0] for c in uc.CASES])
def test_float32_run_of_the_restatement_is_within_the_bounds(case):
    worst = _worst(case, None)
    print('float32 numpy run, %s: %s' % (case[0], {k: round(x, 3) for k, x in worst.items()}))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize('mutation', uc.MUTATIONS)
def test_mutated_updates_exceed_a_bound_tenfold(mutation):
    best = {}
    for case in MUTATED_CASES:
        worst = _worst(case, mutation)
        best[case[0]] = max(worst.values())
    print('mutation %s: %s' % (mutation, {k: float('%.3g' % x) for k, x in best.items()}))
    assert max(best.values()) >= 10.0, best
    if mutation == 'norm_counts_frozen':
        assert best['frozen'] >= 10.0, best
    if mutation == 'norm_stops_at_48':
        assert all(best[k] >= 10.0 for k in uc.SECOND_LIST), best


def test_adam_step_against_the_restatement():
    """oracle.train.adam_step takes the hyper-parameters' float32 values, as Keras and the device do: on float64
    state it is the restatement up to float64 rounding, and a copy of it on the doubles 0.9 / 0.999 / 1e-3 / 1e-7 -- what it was
    before -- stays below the 5e-6 weight bound of tests/test_gpu_train.py over three steps, so that bound never depended on
    the choice."""
    case = uc.BY_NAME['d2_w32']
    w, o32, _ = _oracles(case[0])
    names = list(w)
    g = {k: np.asarray(o32[2][k], np.float64) for k in names}
    w64 = {k: np.asarray(w[k], np.float64) for k in names}
    st = {'t': 0, 'm': {}, 'v': {}}
    wd = {k: a.copy() for k, a in w64.items()}
    md, vd = ({k: np.zeros_like(a) for k, a in w64.items()} for _ in range(2))
    worst = 0.0
    for step in range(3):
        before = ({k: a.copy() for k, a in w64.items()}, {k: st['m'].get(k, np.zeros_like(w64[k])).copy() for k in names},
                  {k: st['v'].get(k, np.zeros_like(w64[k])).copy() for k in names})
        gnorm = adam_step(w64, g, st)
        for k in names:
            (mr, _), (vr, _), (wr, _) = uc.restate(before[0][k], before[1][k], before[2][k], g[k], gnorm, step, uc.DEFAULT,
                                                   st['m'][k], st['v'][k])
            assert np.allclose(st['m'][k], mr, rtol=1e-13, atol=0) and np.allclose(st['v'][k], vr, rtol=1e-13, atol=0)
            assert np.abs(w64[k] - wr).max() < 1e-15
        # the same three steps on the double constants
        scale = 5.0 / gnorm if gnorm >= 5.0 else 1.0
        t = step + 1
        lr_t = 1e-3 * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t)
        for k in names:
            gs = g[k] * scale
            md[k] = 0.9 * md[k] + (1 - 0.9) * gs
            vd[k] = 0.999 * vd[k] + (1 - 0.999) * gs * gs
            wd[k] = wd[k] - lr_t * md[k] / (np.sqrt(vd[k]) + 1e-7)
            worst = max(worst, float(np.abs(wd[k] - w64[k]).max()))
    print('double constants against float32 constants, weights after three steps: %.3g' % worst)
    assert 0 < worst < 0.1 * 5e-6


@pytest.mark.parametrize('kind,V,depth', uc.HEAD_CASES, ids=['%s_v%d_d%d' % c for c in uc.HEAD_CASES])
def test_saturated_head_classes(kind, V, depth):
    cfg, w, (sidx, dec_in, dec_out, wts) = uc.saturated(kind, V, depth)
    assert cfg.width == 32 and dec_out.shape[0] <= 6 and dec_out.shape[1] <= 10
    (_, _, g32), _, p32 = uc.head_oracle(kind, V, depth, 'float32')
    (_, _, g64), _, p64 = uc.head_oracle(kind, V, depth, 'float64')
    on = wts > 0
    c32, c64 = uc.classes(p32[on]), uc.classes(p64[on])
    assert (c64 != -9).all() and np.array_equal(c32, c64)
    assert np.array_equal(uc.classes(p64[on], 4.0), c64)            # no float64 probability within a factor 4 of a threshold
    share = {c: float((c64 == c).mean()) for c in (-1, 0, 1)}
    if kind == 'mixed':
        assert min(share.values()) >= 1 / 8, share
    else:
        assert share[0] == 0 and min(share[-1], share[1]) >= 1 / 8, share
        for k in g64:
            if k != 'E':
                assert not g64[k].any() and not g32[k].any(), k
    # ragged lines: zero-weight rows with a target, -1 rows, and targets on the last index (V = 65: the lane remainder)
    assert ((dec_out >= 0) & ~on).any() and (dec_out < 0).any() and not on[dec_out < 0].any()
    assert (dec_out[on] == V - 1).any() and (dec_out[on] < V - 1).any()
    for k in w:
        if k.endswith(('_K', '_R')) or k.startswith('att_'):
            assert not w[k].any(), k
