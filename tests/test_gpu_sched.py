"""Scheduled sampling on the device (tests/sched_cases.py): the mix kernel alone on constructed and random rows, the sampled step
following the device against the float64 oracle (indices exactly outside the left-out rule, loss and gradients within
tests/grad_noise_cases.py's constants on the last mix), the sequential equivalence, and the entry's contract."""
import numpy as np
import pytest

from tests import grad_noise_cases as gn
from tests import sched_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def engine():
    from cor_asv_ann_amd.engine import HipEngine
    eng = HipEngine(1, 32, 40)
    yield eng
    eng.close()


# ---- the kernel alone ----
@pytest.mark.parametrize('V', sc.KERNEL_V)
def test_constructed_rows(engine, V):
    """What the definition says of every constructed row, whatever the padding columns hold: ties to the lower index, never index
    0, the gold value on a NaN row, an all -inf row, gold -1 and u = 0; ratio 0 leaves every row, ratio 1 replaces every eligible one."""
    rows = sc.constructed_rows(V)
    x = np.stack([r[1] for r in rows])
    gold, u = np.array([r[2] for r in rows], np.int32), np.array([r[3] for r in rows], np.int32)
    b = np.arange(len(rows), dtype=np.int32)
    for pad in (float('nan'), float('inf'), 0.0):
        for pick in ('greedy', 'sample'):
            assert np.array_equal(engine.debug_sched_rows(x, gold, b, u, ratio=0.0, seed=3, step_id=4, pick=pick, pad_value=pad), gold)
            got = engine.debug_sched_rows(x, gold, b, u, ratio=1.0, seed=3, step_id=4, pick=pick, pad_value=pad)
            want = sc.mix_rows(x, gold, b, u, 3, 4, 1.0, pick)
            for (name, xr, g, _, fact), mix, ref in zip(rows, got, want['mix']):
                if fact == 'gold':
                    assert mix == g, (pad, pick, name)
                elif pick == 'greedy':
                    assert mix == fact == ref, (pad, pick, name)
                else:
                    assert 1 <= mix < V and np.isfinite(xr[mix]), (pad, pick, name)        # (replaced: among the drawable candidates)


@pytest.mark.parametrize('V', sc.KERNEL_V)
def test_random_rows_coins_and_picks(engine, V):
    """Random rows at ratio 0.5 over a (seed, step_id) grid with step_id >= 2^32: which rows are replaced is the helper's coin bit for
    bit (a replaced row differs from its gold value by construction), the greedy pick is exact, the sampled pick is draw_rows'
    outside left_out's rule."""
    x, gold, b, u = sc.random_rows(V)
    mark = np.where(gold >= 0, 0, -1).astype(np.int32)     # (a gold value that no pick equals: the coin shows in every eligible row)
    left = n = 0
    for seed, step_id in sc.KERNEL_GRID:
        for pick, tau in sc.KERNEL_DRAWS:
            got = engine.debug_sched_rows(x, mark, b, u, ratio=0.5, seed=seed, step_id=step_id, pick=pick, temperature=tau, pad_value=float('nan'))
            want = sc.mix_rows(x, mark, b, u, seed, step_id, 0.5, pick, tau)
            assert np.array_equal(got != mark, want['replaced']), (seed, step_id, pick)
            assert 0 < want['replaced'].sum() < len(x)
            if pick == 'greedy':
                assert np.array_equal(got, want['mix'])
            else:
                out = sc.sampled_left_out(x.astype(np.float64), x, want['u2'], tau)
                assert np.array_equal(got[~out], want['mix'][~out]), (seed, step_id, tau)
                left += int((out & want['replaced']).sum()); n += int(want['replaced'].sum())
    assert left <= sc.LEFT_OUT_CAP * n, (left, n)


def test_bad_rows_arguments_are_refused(engine):
    from cor_asv_ann_amd._native import NativeError
    x, gold, b, u = sc.random_rows(12, 5)
    for kw in (dict(ratio=-0.1), dict(ratio=1.5), dict(ratio=float('nan')), dict(pick=2), dict(pick='sample', temperature=0.0),
               dict(pick='sample', temperature=float('inf'))):
        with pytest.raises(NativeError) as err:
            engine.debug_sched_rows(x, gold, b, u, **kw)
        assert err.value.code == -1, kw


# ---- the step ----
def _session(case, deterministic=0, persistent=1):
    from cor_asv_ann_amd.engine import HipEngine
    name, d, W, V, lens, keep, flags, with_masks = case
    eng = HipEngine(d, W, V, **{f: True for f in flags})
    eng.set_weights(sc.build(case)[1])
    eng.set_option('persistent', persistent)
    eng.set_option('deterministic', deterministic)
    eng.train_begin()
    return eng


def _sampled(case, mode=2, deterministic=0, persistent=1, **kw):
    """(loss, norm, mixes, grads) of one sampled step in a fresh session."""
    eng = _session(case, deterministic, persistent)
    try:
        kw = dict(dict(seed=sc.SEED, step_id=sc.STEP_ID), **kw)
        loss, norm, mixes = eng.train_step_sampled(*sc.build(case)[3], mode=mode, **kw)
        grads = eng.train_gradients()
        eng.train_end()
        return float(loss), float(norm), mixes, grads
    finally:
        eng.close()


@pytest.mark.parametrize('case', sc.STEP_CASES, ids=sc.STEP_IDS)
def test_sampled_step_follows_the_oracle(case):
    """Slice p - 1 of the device's mixes (gold for p = 1) through the float64 oracle and the definition gives slice p, exactly outside
    the left-out rule and within its cap; persistent 1 and 0 give identical mixes; loss, norm and gradients are the float64 oracle's on
    the last slice within the train step's noise constants."""
    cfg, w, inputs, batch = sc.build(case)
    gold = batch[2]
    for pick, tau in (('greedy', 1.0), ('sample', 0.7)):
        loss, norm, mixes, grads = _sampled(case, ratio=0.5, pick=pick, passes=2, temperature=tau, persistent=1)
        per_step = _sampled(case, ratio=0.5, pick=pick, passes=2, temperature=tau, persistent=0)
        assert np.array_equal(per_step[2], mixes), pick
        assert mixes.shape == (2,) + gold.shape and (mixes[-1] != gold).any()
        cur = gold
        for p in range(2):
            want, out = sc.next_mix(case, cur, gold, 0.5, pick, tau)
            print('%s %s pass %d: %d of %d positions left out, %d replaced' % (case[0], pick, p + 1, out.sum(), out.size, (mixes[p] != gold).sum()))
            assert out.sum() <= sc.LEFT_OUT_CAP * out.size
            assert np.array_equal(mixes[p][~out], want[~out]), (pick, p, mixes[p], want)
            assert ((mixes[p] == gold) | ((mixes[p] >= 1) & (mixes[p] < cfg.voc_size))).all()
            cur = mixes[p]
        last = sc.oracle_inputs(case, mixes[-1])
        o64, o32 = gn.oracle(cfg, w, last, np.float64), gn.oracle(cfg, w, last, np.float32)
        for got in ((loss, norm, grads), (per_step[0], per_step[1], per_step[3])):
            r = gn.ratios(got, o32, o64)
            seen = {k: v for k, v in r.items() if k not in gn.ZERO_GRADIENTS}
            print('%s %s: largest rms ratio %.2f (%s), largest max ratio %.2f (%s)' % (
                case[0], pick, max(v[0] for v in seen.values()), max(seen, key=lambda k: seen[k][0]),
                max(v[1] for v in seen.values()), max(seen, key=lambda k: seen[k][1])))
            bad = {k: v for k, v in seen.items() if v[0] > gn.C_RMS or v[1] > gn.C_MAX}
            assert not bad, (pick, bad)
            for k in gn.ZERO_GRADIENTS:
                assert gn.within_old_bound(got[2][k], o64[2][k], o64[1]), (pick, k)


def test_give_up_path_gives_the_same_mix(capfd):
    """persistent = 2: a workgroup of every forward recurrence leaves, its peers give up (width 64: two workgroups per layer, so
    there is a peer), the step is redone with per-step launches -- the mixes of persistent = 0, its loss and norm as
    tests/test_gpu_train.py holds the hard step's (the backward pass adds by float atomics: no equal bits)."""
    case = sc.STEP_CASES[4]
    want = _sampled(case, ratio=0.5, passes=2, persistent=0)
    capfd.readouterr()
    got = _sampled(case, ratio=0.5, passes=2, persistent=2)
    assert 'gave up waiting' in capfd.readouterr().err
    assert np.array_equal(got[2], want[2])
    assert abs(got[0] - want[0]) < 1e-8 * abs(want[0]) and abs(got[1] - want[1]) < 2e-5 * want[1]


def test_sequential_equivalence():
    """U = 6, greedy, ratio 0.5: with passes = 5 the last slice is the sequential procedure's input; with passes = 2 it agrees with it
    on positions <= 2."""
    case = sc.SEQ_CASE
    gold = sc.build(case)[3][2]
    seq, out = sc.sequential(case, gold, 0.5)
    assert not out.any() and gold.shape[1] == 6
    five = _sampled(case, ratio=0.5, passes=5)[2]
    assert np.array_equal(five[-1], seq)
    two = _sampled(case, ratio=0.5, passes=2)[2]
    assert np.array_equal(two[-1][:, :3], seq[:, :3])
    for p in range(5):
        assert np.array_equal(five[p][:, :p + 2], seq[:, :p + 2]), p


# ---- the contract ----
def _equal(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize('name', ['d2_w32_v12', 'd2_w64_v40_masks'])
def test_ratio_0_is_the_hard_step_bit_for_bit(name):
    case = sc.STEP_CASES[sc.STEP_IDS.index(name)]
    batch = sc.build(case)[3]
    eng = _session(case, deterministic=1)
    try:
        hard = eng.train_step(*batch, mode=2)
        hard_grads = eng.train_gradients()
    finally:
        eng.close()
    loss, norm, mixes, grads = _sampled(case, deterministic=1, ratio=0.0, passes=3)
    assert np.float64(loss).tobytes() == np.float64(hard[0]).tobytes() and norm == hard[1] and _equal(grads, hard_grads)
    assert mixes.shape[0] == 3 and all(np.array_equal(m, batch[2]) for m in mixes)


def test_deterministic_sampled_steps_repeat_bit_for_bit():
    case = sc.STEP_CASES[4]
    a = _sampled(case, deterministic=1, ratio=0.5, passes=2, pick='sample')
    b = _sampled(case, deterministic=1, ratio=0.5, passes=2, pick='sample')
    assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and _equal(a[3], b[3])
    assert (a[2][-1] != sc.build(case)[3][2]).any() and np.isfinite(a[0])
    # ... and the ordered embedding gradient is the one of the last mix: the float64 oracle's within the noise constants
    cfg, w, _, _ = sc.build(case)
    last = sc.oracle_inputs(case, a[2][-1])
    r = gn.ratios((a[0], a[1], a[3]), gn.oracle(cfg, w, last, np.float32), gn.oracle(cfg, w, last, np.float64))
    assert r['E'][0] <= gn.C_RMS and r['E'][1] <= gn.C_MAX, r['E']


def test_refusals_leave_the_session_untouched_and_no_state_leaks():
    from cor_asv_ann_amd._native import NativeError
    case = sc.STEP_CASES[1]
    batch = sc.build(case)[3]
    eng, ref = _session(case, deterministic=1), _session(case, deterministic=1)
    try:
        assert eng.train_step(*batch, mode=1) == ref.train_step(*batch, mode=1)
        before = (eng.train_state(), eng.train_gradients())
        assert before[0][2] == 1
        good = dict(mode=1, ratio=0.5, passes=1, pick='greedy', temperature=1.0)
        for change in (dict(mode=0), dict(ratio=-0.01), dict(ratio=1.01), dict(ratio=float('nan')), dict(passes=0), dict(passes=9),
                       dict(pick=2), dict(pick=-1), dict(pick='sample', temperature=0.0), dict(pick='sample', temperature=float('nan')),
                       dict(pick='sample', temperature=float('inf'))):
            with pytest.raises(NativeError) as err:
                eng.train_step_sampled(*batch, **dict(good, **change))
            assert err.value.code == -1, change                 # CASV_ERR_ARG
            (m, v, step), grads = eng.train_state(), eng.train_gradients()
            assert step == 1 and _equal(grads, before[1]) and _equal(m, before[0][0]) and _equal(v, before[0][1]), change
        for null in ('p', 'out'):
            import ctypes
            from cor_asv_ann_amd import _native as nv
            p = eng._sched_params(1, 0, 0.5, 'greedy', 1, 1.0)
            out = np.empty((1,) + batch[2].shape, np.int32)
            loss = ctypes.c_double()
            idx = np.ascontiguousarray(batch[0][:, :, None])
            B, T, A = idx.shape
            rc = eng.lib.casv_train_step_sampled(eng.handle, 1, B, T, batch[2].shape[1], A, nv.ptr(idx), None, nv.ptr(batch[2]), nv.ptr(batch[3]),
                                                 nv.ptr(batch[4]), None, None, None, None if null == 'p' else ctypes.byref(p),
                                                 None if null == 'out' else nv.ptr(out), ctypes.byref(loss), None)
            assert rc == -1, null
            assert eng.train_state()[2] == 1
        # sampled steps without an update, then the same hard step as in the session that never sampled: equal bits
        mixes = eng.train_step_sampled(*batch, mode=2, ratio=0.5, seed=sc.SEED, step_id=1, passes=2)[2]
        assert (mixes[-1] != batch[2]).any()
        eng.train_step_sampled(*batch, mode=2, ratio=1.0, seed=5, step_id=9, passes=1, pick='sample')
        a, b = eng.train_step(*batch, mode=1), ref.train_step(*batch, mode=1)
        assert a == b and _equal(eng.train_gradients(), ref.train_gradients()) and _equal(eng.train_weights(), ref.train_weights())
        eng.train_end(); ref.train_end()
    finally:
        eng.close(); ref.close()


def test_train_with_a_sample_schedule(tmp_path, monkeypatch):
    """A constant ratio 0.5 completes with finite losses, repeats bit for bit under `seed` and `deterministic`, and ends at other
    weights than ratio 0."""
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence
    from cor_asv_ann_amd.synthetic import make_lines
    lines, _ = make_lines(320, 9, 5, voc_size=24)
    corpus = str(tmp_path / 'train.tsv')
    with open(corpus, 'w') as f:
        f.write(''.join('%s\t%s\n' % (l[:-1], l[:-1]) for l in lines))
    runs = {}
    for sub, kw in (('zero', dict(sample_schedule=0.0)), ('half', dict(sample_schedule=0.5, sample_passes=2)), ('again', dict(sample_schedule=0.5, sample_passes=2))):
        (tmp_path / sub).mkdir()
        monkeypatch.chdir(tmp_path / sub)
        s2s = Sequence2Sequence(progbars=False)
        s2s.depth, s2s.width, s2s.batch_size, s2s.epochs = 2, 32, 32, 2
        s2s.seed, s2s.deterministic = 11, True
        s2s.configure()
        s2s.train([corpus], **kw)
        assert len(s2s.history) == 2 and all(np.isfinite(h['loss']) and np.isfinite(h['val_loss']) for h in s2s.history), (sub, s2s.history)
        runs[sub] = s2s
    assert runs['again'].history == runs['half'].history and _equal(runs['again']._weights, runs['half']._weights)
    assert not _equal(runs['half']._weights, runs['zero']._weights)
