"""The train step behind its gradients, on the device (tests/update_cases.py; tests/test_update_bounds.py shows without a GPU that
the bounds have teeth): the norm, the Adam update as an elementwise function of what the device itself holds, the clip decision
bit for bit, and the loss head and the embedding regulariser at their edges against float64."""
import numpy as np
import pytest

from cor_asv_ann_amd import _native as nv
from tests import grad_noise_cases as gn
from tests import update_cases as uc

pytestmark = pytest.mark.gpu


def _bits_equal(a, b):
    return all(np.array_equal(np.asarray(a[k], np.float32).view(np.uint32), np.asarray(b[k], np.float32).view(np.uint32)) for k in a) \
        and set(a) == set(b)


def _assert_within(r, what):
    print('%s: norm %.3g m %.3f v %.3f w %.3f scale %.9g' % (what, r['norm'], r['m'], r['v'], r['w'], r['scale']))
    assert r['norm'] <= 1.0 and r['m'] <= 1.0 and r['v'] <= 1.0 and r['w'] <= 1.0 and r['moved'] == 0, (what, r)


# ------------------------------------------------------------------------------------------------------------------ 1. the update
@pytest.mark.parametrize('deterministic', (0, 1))
@pytest.mark.parametrize('case', uc.CASES, ids=[c[0] for c in uc.CASES])
def test_update_within_derived_bounds(case, deterministic):
    s = uc.Session(case, deterministic)
    try:
        eng = s.eng
        assert len(s.names) == uc.TENSORS[case[0]] and (len(s.names) > uc.MULTI_MAX) == (case[0] in uc.SECOND_LIST)
        shapes = {k: eng.shapes[k] for k in s.names}
        for hname, hyper in uc.HYPERS.items():
            # two consecutive steps from zero moments
            s.begin(hyper)
            for n in range(2):
                before, after, g, gnorm, step = s.step()
                assert step == n and (n or not any(before[q][k].any() for q in (1, 2) for k in s.names))
                r = uc.check(before, after, g, gnorm, step, hyper, s.names)
                assert (r['scale'] < 1) == uc.CLIPS[hname], (hname, gnorm)
                _assert_within(r, '%s det %d %s zero moments step %d' % (case[0], deterministic, hname, step))
            # seeded moments: every step count under the default set, two of them (in turn) under each other set
            for i, step0 in enumerate(uc.STEPS):
                if hname != 'default' and i % 3 != list(uc.HYPERS).index(hname) % 3:
                    continue
                s.begin(hyper)
                m, v = uc.seeded_moments(shapes, 100 + i)
                eng.set_train_state(m, v, step0)
                before, after, g, gnorm, step = s.step()
                assert step == step0 and _bits_equal(before[1], m) and _bits_equal(before[2], v)
                r = uc.check(before, after, g, gnorm, step, hyper, s.names)
                _assert_within(r, '%s det %d %s seeded step %d' % (case[0], deterministic, hname, step0))
                zeros = sum(int(((m[k] == 0) & (v[k] == 0) & (g[k] == 0)).sum()) for k in s.names)
                assert zeros > 0 or case[7] is False, 'no element with m = v = g = 0'
            # frozen tensors: unchanged bit for bit, no optimizer state
            for k in eng.shapes:
                if k not in s.names:
                    assert np.array_equal(after[0][k].view(np.uint32), np.asarray(s.w[k], np.float32).reshape(after[0][k].shape).view(np.uint32)), k
                    assert k not in after[1] and k not in after[2]
                    buf = np.empty(eng.pshapes[k], np.float32)
                    for which in (0, 1):
                        assert eng.lib.casv_train_get_state(eng.handle, k.encode(), which, nv.ptr(buf), buf.size) != 0, k
            # dead-unit padding: w, m, v stay exactly 0 there (the last session's moments were seeded)
            if eng.pwidth != eng.width:
                padded = 0
                for k in s.names:
                    pad = uc.padding_of(eng, k)
                    padded += int(pad.sum())
                    for what in 'wgmv':
                        a = uc.raw_read(eng, what, k)
                        assert not a[pad].any(), (k, what)
                assert padded > 0
        assert case[0] != 'w50_padded' or eng.pwidth == 64
        assert bool(case[10]) == (len(s.names) < len(eng.shapes))
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 2. the clip decision
@pytest.mark.parametrize('name', ('d2_w32', 'd8_w32'))
def test_clip_decision_bit_for_bit(name):
    case = uc.BY_NAME[name]
    s = uc.Session(case, 1)
    try:
        runs = []
        hyper = dict(uc.DEFAULT, clipnorm=0.0)
        for k in range(4):
            s.begin(hyper)
            runs.append(s.step() + (hyper,))
            if k == 0:
                n32 = np.float32(runs[0][3])
                clips = [np.nextafter(n32, np.float32(np.inf)), n32, np.nextafter(n32, np.float32(0))]
                assert clips[0] > n32 > clips[2] > 0
            if k < 3:
                hyper = dict(uc.DEFAULT, clipnorm=float(clips[k]))
        before0, after0, g0, gn0 = runs[0][:4]
        for k in (1, 2, 3):             # the deterministic mode's own promise
            assert _bits_equal(runs[k][2], g0) and runs[k][3] == gn0, k
            assert all(_bits_equal(runs[k][0][q], before0[q]) for q in range(3))
        for k in (1, 2):                # clipnorm one float32 above the norm: no clip; at the norm: clipnorm / norm is exactly 1
            assert all(_bits_equal(runs[k][1][q], after0[q]) for q in range(3)), k
        before, after, g, gnorm, step, hyper = runs[3]
        r = uc.check(before, after, g, gnorm, step, hyper, s.names)
        assert r['scale'] < 1
        _assert_within(r, '%s clipnorm one float32 below the norm' % name)
        nonzero = np.concatenate([(after0[1][k] != 0).ravel() for k in s.names])
        differs = np.concatenate([(after[1][k] != after0[1][k]).ravel() for k in s.names])
        assert differs[nonzero].mean() > 0.5, differs[nonzero].mean()
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 3. the loss head
def _noise_ok(r, what):
    bad = {k: v for k, v in r.items() if v[0] > gn.C_RMS or v[1] > gn.C_MAX}
    print('%s: largest rms ratio %.3g, largest max ratio %.3g' % (what, max(v[0] for v in r.values()), max(v[1] for v in r.values())))
    assert not bad, (what, bad)


@pytest.mark.parametrize('kind,V,depth', uc.HEAD_CASES, ids=['%s_v%d_d%d' % c for c in uc.HEAD_CASES])
def test_loss_head_at_its_clip_edges(kind, V, depth):
    cfg, w, batch = uc.saturated(kind, V, depth)
    o32, ce32, _ = uc.head_oracle(kind, V, depth, 'float32')
    o64, ce64, _ = uc.head_oracle(kind, V, depth, 'float64')
    for path in ('fused', 'stepwise'):
        for det in (0, 1):
            got = uc.head_device(cfg, w, batch, path, det)
            what = '%s V %d depth %d %s det %d' % (kind, V, depth, path, det)
            _noise_ok({'loss_ce': gn.ratios((got[0][0], 0.0, {}), (ce32, 0.0, {}), (ce64, 0.0, {}))['loss']}, what + ' mode 0')
            _noise_ok(gn.ratios(got[2], o32, o64), what + ' mode 2')
            if kind == 'all_clipped':
                for k, g in got[2][2].items():
                    assert k == 'E' or not np.asarray(g).any(), (what, k)
                ratio, r = uc.regulariser_ratios(w['E'], got[2][0] - got[0][0], got[2][0], got[2][2]['E'])
                print('%s regulariser: loss %.3g, dE rms %.3g max %.3g' % (what, ratio, r[0], r[1]))
                assert ratio <= gn.C_MAX and r[0] <= gn.C_RMS and r[1] <= gn.C_MAX, (what, ratio, r)


@pytest.mark.parametrize('variant', uc.REG_VARIANTS)
def test_regulariser_on_its_own(variant):
    """The regulariser's loss as mode-2 loss - mode-0 loss (no dropout masks), its gradient as dE of the same batch with every
    weight 0, where nothing else reaches dE."""
    V, depth = 65, 1
    cfg, w, batch = uc.saturated('mixed', V, depth)
    _, _, zero_batch = uc.saturated('mixed', V, depth, 'zero')
    w = dict(w, E=uc.regulariser_embedding(V, variant))
    rows = np.sqrt((w['E'].astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(rows / rows[0] - 1).max() < 2.0 ** -23
    for path in ('fused', 'stepwise'):
        for det in (0, 1):
            got = uc.head_device(cfg, w, batch, path, det)
            zero = uc.head_device(cfg, w, zero_batch, path, det, modes=(2,))
            ratio, r = uc.regulariser_ratios(w['E'], got[2][0] - got[0][0], got[2][0], zero[2][2]['E'])
            print('%s %s det %d: loss %.3g, dE rms %.3g max %.3g' % (variant, path, det, ratio, r[0], r[1]))
            assert ratio <= gn.C_MAX and r[0] <= gn.C_RMS and r[1] <= gn.C_MAX, (variant, path, det, ratio, r)
            assert all(k == 'E' or not np.asarray(g).any() for k, g in zero[2][2].items())
            # the zero-weight batch: no cross-entropy, so its mode-2 loss is the regulariser alone
            ratio0, _ = uc.regulariser_ratios(w['E'], zero[2][0], zero[2][0], zero[2][2]['E'])
            assert ratio0 <= gn.C_MAX, (variant, path, det, ratio0)
