"""Sampling under a cut (top_k, top_p) on the device (csrc/sample_kernels.hip: sample_cut_kernel; csrc/sched_kernels.hip:
sched_mix_cut_kernel; casv_decode_sample_cut, casv_debug_sample_cut_rows, casv_train_step_sampled_cut, casv_debug_sched_cut_rows;
DESIGN.md section 4.8, items 11 to 13): the kernel alone against the float64 restatement, the bit identities with the entries without
a cut, the decode call against the oracle forced along the device's sequence, scheduled sampling, and the facade.  Cases, references
and bounds: tests/sample_cut_cases.py, held on the CPU by tests/test_sample_cut_cases.py."""
import ctypes
import glob
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

os.environ.setdefault('CASV_POISON', '1')      # read once by the library, at its first allocation

from tests import sample_cases as sa
from tests import sample_cut_cases as cu
from tests import sched_cases as sch
from tests import score_cases as sc
from tests.decode_noise_cases import C_MAX

U_SWEEP = np.concatenate([np.array([0.0, 1 - 2.0 ** -24]), (np.arange(30) + 0.5) / 30]).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same(a, b):
    """Bit for bit."""
    return all(np.array_equal(np.ascontiguousarray(x).view(np.int32), np.ascontiguousarray(y).view(np.int32)) for x, y in zip(a, b))


@pytest.fixture(scope='module')
def head_engine():
    from cor_asv_ann_amd.engine import HipEngine
    eng = HipEngine(1, 32, 40)
    yield eng
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ a. the kernel alone
def _check_rows(eng, x, tau, cut, name, u=None, streams=None, samples=None, step=0, seed=0, pads=sc.PADS):
    """One batch of rows under the padding values: the pick where it is not left out, the head's bits, logq, the feedback rows."""
    R, V = x.shape
    s_ = np.arange(R) if streams is None else streams
    n_ = np.zeros(R, np.int64) if samples is None else samples
    uu = sa.uniform(seed, s_, n_, step) if u is None else np.asarray(u, np.float32)
    d64, d32 = cu.draw_rows(x, uu, tau, cut), cu.draw_rows(x, uu, tau, cut, np.float32)
    lo, _ = cu.left_out(uu, d64, d32, cu.KERNEL_FLOOR)
    first = None
    for pad in pads:
        got = eng.debug_sample_cut_rows(x, tau, cut[0], cut[1], seed=seed, step=step, streams=streams, samples=samples, u=u, pad_value=pad)
        first = first or got
        assert _same(got, first), (name, pad)                # no output bit moves with the padding columns
    idx, logp, logq, fb = first
    valid = d64['valid']
    assert np.array_equal(idx[valid & ~lo], d64['idx'][valid & ~lo]), (name, idx, d64['idx'], lo)
    assert (idx[~valid] == 1).all() and np.isnan(logp[~valid]).all() and np.isnan(logq[~valid]).all(), name
    rows = np.nonzero(valid)[0]
    assert (idx[rows] >= 1).all() and (x[rows, idx[rows]] > -np.inf).all(), name
    assert np.array_equal(_bits(fb), _bits(sa.onehot_rows(idx, valid, V))), name       # exactly one-hot: Vp - 1 exact zeros
    head = eng.debug_score_rows(x, idx)[0]                  # logp: the bits of the scoring head for that index as target
    finite = valid & np.isfinite(x.max(axis=1))
    assert np.array_equal(_bits(head[finite]), _bits(logp[finite])) and np.isnan(logp[valid & ~finite]).all(), name
    ok = rows[d64['cand'][rows, idx[rows]] & ~lo[rows]]     # logq of the index the device drew, in float64, over the reference's kept set
    with np.errstate(divide='ignore', invalid='ignore'):
        want = np.log(d64['w'][ok, idx[ok]] / d64['w'][ok].sum(axis=1))
    worst = float(sc.units_or_inf(logq[ok], want).max(initial=0.0)) / (4 * sc.e_np())
    print('%s: %d rows, %d left out, logq %.3f of the bound' % (name, R, int(lo.sum()), worst))
    assert worst <= 1, name
    return first, lo


@pytest.mark.parametrize('c', cu.KERNEL_CASES, ids=cu.KERNEL_IDS)
def test_kernel_against_float64_and_the_head(head_engine, c):
    V, R, cut, tau, _ = c
    x, streams, samples, step, seed = cu.kernel_case(c)                 # (stream ids beyond 2^32 among them)
    got, lo = _check_rows(head_engine, x, tau, cut, str(c), streams=streams, samples=samples, step=step, seed=seed,
                          pads=sc.PADS if V <= 640 else sc.PADS[:2])
    assert lo.sum() <= cu.cap_rows(R), (int(lo.sum()), R)
    u = sa.uniform(seed, streams, samples, step)
    assert _same(head_engine.debug_sample_cut_rows(x, tau, cut[0], cut[1], u=u), got)        # the uniforms handed in: the same bits
    assert head_engine.stat('sample_cut_rows') == (4 if V <= 2048 else 3)


def test_kernel_on_constructed_rows(head_engine):
    for name, x, cut, tau, facts in cu.constructed_rows():
        rows = np.repeat(x[None], len(U_SWEEP), axis=0)
        (idx, _, _, _), lo = _check_rows(head_engine, rows, tau, cut, name, u=U_SWEEP, pads=sc.PADS[:2])
        if facts['valid']:
            # u = 0 and u = 1 - 2^-24 are compared (but at top_p one float32 below 1 the weightless places' masses of exactly 1 lie
            # within any margin of it: those rows are held by their facts alone, which need none)
            assert not lo[:2].any() or name.startswith('minus_inf_members'), name
            if 'only' in facts:
                assert set(idx.tolist()) <= set(facts['only']), (name, sorted(set(idx.tolist())))
            if 'never' in facts:
                assert not set(idx.tolist()) & set(facts['never']), name
            assert 0 not in idx


@pytest.mark.parametrize('V', (12, 40, 65, 640, 4096))
def test_bit_identities_with_the_kernel_without_a_cut(head_engine, V):
    eng = head_engine
    rng = np.random.default_rng(V)
    R = 9
    x = (rng.standard_normal((R, V)) * (3.0 if V < 4096 else 8.0)).astype(np.float32)
    x[1, 3:9] = x[1, 3]                                                   # a tie group
    kw = dict(seed=11, step=3, streams=rng.integers(0, 2 ** 40, R).astype(np.int64))
    for tau in (0.5, 1.0):
        for k in (0, 1, 8, 64):                                           # (k, 1.0) is sample_kernel at top_k = k
            assert _same(eng.debug_sample_cut_rows(x, tau, k, 1.0, **kw), eng.debug_sample_rows(x, tau, k, **kw)), (V, tau, k)
        assert _same(eng.debug_sample_cut_rows(x, tau, 0, cu.SMALLEST_P, **kw), eng.debug_sample_rows(x, tau, 1, **kw)), (V, tau)
        for cut in ((0, 0.5), (0, 0.9), (5, 0.9)):                        # a row whose nucleus has n members: the bits of top_k = n
            got = eng.debug_sample_cut_rows(x, tau, cut[0], cut[1], **kw)
            d64, d32 = cu.draw_rows(x, np.zeros(R), tau, cut), cu.draw_rows(x, np.zeros(R), tau, cut, np.float32)
            sure = np.nonzero(d64['n'] == d32['n'])[0]
            assert len(sure) >= R - 2
            for r in sure:
                n = int(d64['n'][r])
                one = dict(kw, streams=kw['streams'][r:r + 1])
                # (n: the member count of the float64 and float32 restatements alike; a device that counts n +- 1 at a border closer
                # than either sees fails here and is looked at by hand)
                want = eng.debug_sample_rows(x[r:r + 1], tau, n, **one) if n <= 64 else eng.debug_sample_cut_rows(x[r:r + 1], tau, n, 1.0, **one)
                assert _same([g[r:r + 1] for g in got], want), (V, tau, cut, r, n)


@pytest.mark.parametrize('V,cut', [(40, (0, 0.9)), (65, (5, 0.9)), (640, (100, 1.0)), (4096, (0, 0.9))])
def test_a_row_never_depends_on_its_launch(head_engine, V, cut):
    """The same rows alone, in a batch of 5 and of 1000, in reversed order, and under every rows-per-workgroup form."""
    eng = head_engine
    rng = np.random.default_rng(V + 1)
    x5 = (rng.standard_normal((5, V)) * (3.0 if V < 4096 else 8.0)).astype(np.float32)
    u5 = rng.random(5).astype(np.float32)
    R = 1000 if V <= 640 else 50
    rows = rng.integers(0, 5, R)
    rows[:5] = np.arange(5)
    five = eng.debug_sample_cut_rows(x5, 0.8, cut[0], cut[1], u=u5)
    forms = {}
    try:
        for limit in (0, 1, 2, 3, 4):
            eng.set_option('sample_cut_rows', limit)
            many = eng.debug_sample_cut_rows(x5[rows], 0.8, cut[0], cut[1], u=u5[rows])
            forms.setdefault(eng.stat('sample_cut_rows'), limit)
            assert _same(many, [g[rows] for g in five]), (V, limit)
            back = eng.debug_sample_cut_rows(x5[rows][::-1], 0.8, cut[0], cut[1], u=u5[rows][::-1])
            assert _same([g[::-1] for g in back], many), (V, limit)
            for r in range(5):
                assert _same(eng.debug_sample_cut_rows(x5[r:r + 1], 0.8, cut[0], cut[1], u=u5[r:r + 1]), [g[r:r + 1] for g in five]), (V, limit, r)
    finally:
        eng.set_option('sample_cut_rows', 0)
    assert sorted(forms) == ([1, 2, 3, 4] if V <= 2048 else [1, 2, 3]), forms


def test_kernel_arguments(head_engine):
    from cor_asv_ann_amd._native import NativeError
    from cor_asv_ann_amd import _native as nv
    eng = head_engine
    x = np.zeros((2, 40), np.float32)
    for kw in (dict(top_k=-1), dict(top_k=4096), dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=1.0001), dict(top_p=np.nan),
               dict(temperature=0.0), dict(temperature=np.inf), dict(step=-1)):
        with pytest.raises(NativeError) as e:
            eng.debug_sample_cut_rows(x, **kw)
        assert e.value.code == -1, kw
    out = [np.empty(2, np.int32), np.empty(2, np.float32), np.empty(2, np.float32), np.empty((2, 64), np.float32)]
    tail = [0, None, None, nv.ptr(x), None, ctypes.c_float(0.0)] + [nv.ptr(o) for o in out]
    p, cut = nv.SampleParams(1, 1.0, 0, 1), nv.SampleCut(5, 0.9)
    assert eng.lib.casv_debug_sample_cut_rows(eng.handle, 2, 40, ctypes.byref(p), None, *tail) == -1                  # NULL cut
    p5 = nv.SampleParams(1, 1.0, 5, 1)
    assert eng.lib.casv_debug_sample_cut_rows(eng.handle, 2, 40, ctypes.byref(p5), ctypes.byref(cut), *tail) == -1     # the cut carries top_k
    assert eng.lib.casv_debug_sample_cut_rows(eng.handle, 2, 40, ctypes.byref(p), ctypes.byref(cut), *tail) == 0
    for bad in (-1, 5):
        with pytest.raises(NativeError):
            eng.set_option('sample_cut_rows', bad)
    eng.profile(True)                                       # timed under the class "sample"
    before = eng.profile_read('sample')['launches']
    eng.debug_sample_cut_rows(x, top_p=0.9)
    assert eng.profile_read('sample')['launches'] == before + 1
    eng.profile(False)


# ------------------------------------------------------------------------------------------------------------------ b. the decode call
def _engine(case, arithmetic=None):
    from cor_asv_ann_amd.engine import HipEngine
    mc = sa.build_model(case)
    eng = HipEngine(case[1], case[2], case[3], **mc['flags'])
    eng.set_weights(mc['w'])
    if arithmetic is not None:
        eng.set_option('arithmetic', arithmetic)
    return eng, mc


@pytest.mark.parametrize('case,tau,cut', cu.MODEL_DRAWS, ids=cu.MODEL_DRAW_IDS)
def test_samples_match_the_oracle_forced_along_them(case, tau, cut):
    eng, mc = _engine(case)
    N, seed = mc['N'], 4242
    try:
        eng.encode(mc['idx'], mc['val'])
        got = eng.decode_sample_cut(N, tau, cut[0], cut[1], seed, want_align=True)
        again = eng.decode_sample_cut(N, tau, cut[0], cut[1], seed, want_align='sparse')
        assert _same(got[:4], again[:4])                                    # two calls with the same seed
        f = cu.check_model(case, got, tau, cut, seed, align=got[4], sparse=again[4])
        print('%s tau=%g cut=%r: %d draws, %d left out, %d wrong, smallest delta that matches every draw %.3g; exp(logp) (rms, max) = '
              '(%.3f, %.3f), alignment rows (%.3f, %.3f), sparse (%.3f, %.3f) units; logq off by %.3g'
              % ((case[0], tau, cut, f['draws'], f['left_out'], f['wrong'], f['need']) + f['logp'] + f['align'] + f['sparse'] + (f['logq'],)))
        assert f['wrong'] == 0
        assert f['left_out'] <= cu.LEFT_OUT_CAP * f['draws']
        assert f['logp'][1] <= C_MAX and f['align'][1] <= C_MAX and f['sparse'][1] <= C_MAX
    finally:
        eng.close()


def _reported(got, b, n):
    k = int(got[3][b, n])
    return got[0][b, n, :k].tolist(), _bits(got[1][b, n, :k]).tolist(), _bits(got[2][b, n, :k]).tolist()


def test_decode_call_identities_and_batches():
    case = sa.BATCH_CASE
    eng, mc = _engine(case)
    idx = mc['idx']
    B = len(idx)
    try:
        eng.encode(idx)
        for k in (0, 1, 7, 64):                                            # (k <= 64, 1.0): casv_decode_sample, every output bit
            a = eng.decode_sample_cut(2, 0.8, k, 1.0, seed=99, want_align=True)
            b = eng.decode_sample(2, 0.8, k, seed=99, want_align=True)
            assert _same(a, b), k
        kw = dict(temperature=0.8, top_k=0, top_p=0.7, seed=99)
        seven = eng.decode_sample_cut(1, **kw)
        eng.encode(idx[3:4])
        alone = eng.decode_sample_cut(1, streams=[3], **kw)
        assert _reported(alone, 0, 0) == _reported(seven, 3, 0)             # alone, and as line 3 of 7
        eng.encode(idx)
        eight = eng.decode_sample_cut(8, **kw)
        for b in range(B):
            assert _reported(eight, b, 0) == _reported(seven, b, 0)         # N = 1 against N = 8
        assert _same(eng.decode_sample_cut(8, **kw)[:4], eight[:4])
        assert not np.array_equal(eng.decode_sample_cut(8, **dict(kw, top_p=1.0))[0], eight[0])         # the nucleus cuts something
    finally:
        eng.close()


def test_decode_refusals_leave_the_next_call_its_bits():
    from cor_asv_ann_amd._native import NativeError
    from cor_asv_ann_amd import _native as nv
    case = sa.BATCH_CASE
    eng, mc = _engine(case)

    def refused(call, code, word=None):
        with pytest.raises(NativeError) as e:
            call()
        assert e.value.code == code and (word is None or word in str(e.value)), str(e.value)
    try:
        refused(lambda: eng.decode_sample_cut(2, top_p=0.9, steps=4), -2, 'casv_encode')
        eng.encode(mc['idx'])
        first = eng.decode_sample_cut(2, top_p=0.9, seed=3)
        B, S = eng.B, 4
        bufs = [np.empty((B * 2, S), np.int32), np.empty((B * 2, S), np.float32), np.empty((B * 2, S), np.float32), np.empty(B * 2, np.int32)]
        ptrs = [nv.ptr(b) for b in bufs] + [None]
        p, cut = nv.SampleParams(1, 1.0, 0, 2), nv.SampleCut(0, 0.9)
        calls = [lambda: eng.decode_sample_cut(2, top_k=-1), lambda: eng.decode_sample_cut(2, top_k=4096), lambda: eng.decode_sample_cut(2, top_p=0.0),
                 lambda: eng.decode_sample_cut(2, top_p=-1.0), lambda: eng.decode_sample_cut(2, top_p=1.5), lambda: eng.decode_sample_cut(2, top_p=np.nan),
                 lambda: eng.decode_sample_cut(0, top_p=0.9), lambda: eng.decode_sample_cut(2, top_p=0.9, temperature=0.0),
                 lambda: eng.decode_sample_cut(2, top_p=0.9, steps=2 * 4096 + 1),
                 lambda: nv.check(eng.lib.casv_decode_sample_cut(eng.handle, ctypes.byref(p), None, S, None, *ptrs)),
                 lambda: nv.check(eng.lib.casv_decode_sample_cut(eng.handle, None, ctypes.byref(cut), S, None, *ptrs)),
                 lambda: nv.check(eng.lib.casv_decode_sample_cut(eng.handle, ctypes.byref(nv.SampleParams(1, 1.0, 3, 2)), ctypes.byref(cut), S, None, *ptrs)),
                 lambda: nv.check(eng.lib.casv_decode_sample_cut(eng.handle, ctypes.byref(p), ctypes.byref(cut), S, None, None, *ptrs[1:]))]
        for k, call in enumerate(calls):
            refused(call, -1)
            assert _same(eng.decode_sample_cut(2, top_p=0.9, seed=3)[:4], first[:4]), k
        refused(lambda: eng.decode_sample(2, top_k=65), -1, 'top_k=65')                         # the entry without a cut is what it was
        dense = eng.decode_sample_cut(2, top_p=0.9, seed=3, want_align=True)                   # the sparse alignments serve B * N rows
        lo, w = eng.alignments_sparse(eng.B * 2, dense[0].shape[2])
        for b in range(eng.B):
            for n in range(2):
                for s in range(int(dense[3][b, n])):
                    row = np.zeros(eng.T + w.shape[2], np.float32)
                    row[lo[b * 2 + n, s]:lo[b * 2 + n, s] + w.shape[2]] = w[b * 2 + n, s]
                    assert np.array_equal(_bits(row[:eng.T]), _bits(dense[4][b, n, s]))
    finally:
        eng.close()


def test_a_nan_row_ends_there_and_leaves_the_others_their_bits():
    """As tests/test_gpu_sample.py: line 1's encoder output is NaN at a position one of its rows attends only after the first step."""
    from cor_asv_ann_amd._native import NativeError, CASV_ERR_NAN
    case = sa.MODEL_CASES[1]
    eng, mc = _engine(case)
    N, S, kw = 2, 8, dict(seed=17, temperature=1.0, top_k=0, top_p=0.8)
    _, enc, states, _ = sa._encoded(case, np.float32)
    enc, states = np.array(enc, np.float32), [np.array(s, np.float32) for s in states[:-1]]
    try:
        eng.set_encoder_outputs(enc, states)
        clean = eng.decode_sample_cut(N, steps=S, want_align=True, **kw)
        inside = clean[4][1] > 0
        first = np.where(inside.any(axis=1), inside.argmax(axis=1), S)
        cand = sorted((first[:, q].min(), q) for q in range(inside.shape[2]) if 1 <= first[:, q].min() < S)
        assert cand, 'no position enters a window after the first step'
        at, q = cand[0]
        bad = enc.copy()
        bad[1, q] = np.nan
        eng.set_encoder_outputs(bad, states)
        with pytest.raises(NativeError) as e:
            eng.decode_sample_cut(N, steps=S, want_align=True, **kw)
        assert e.value.code == CASV_ERR_NAN
        got = e.value.outputs
        hit = False
        for n in range(N):
            k = int(first[n, q])
            if k >= int(clean[3][1, n]):
                assert _reported(got, 1, n) == _reported(clean, 1, n)
                continue
            hit = True
            assert got[3][1, n] == k + 1 and got[0][1, n, k] == 1 and np.isnan(got[1][1, n, k]) and np.isnan(got[2][1, n, k])
            assert got[0][1, n, :k].tolist() == clean[0][1, n, :k].tolist()
        assert hit
        for b in range(len(enc)):
            if b != 1:
                for n in range(N):
                    assert _reported(got, b, n) == _reported(clean, b, n)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------ c. scheduled sampling
@pytest.mark.parametrize('V', (12, 33, 256, 4096))
def test_mix_kernel_draws_what_the_sampling_kernel_draws(head_engine, V):
    eng = head_engine
    x, gold, b, u = sch.random_rows(V)
    mark = np.where(gold >= 0, 0, -1).astype(np.int32)
    left = n = 0
    for (seed, step_id), tau, cut in zip(sch.KERNEL_GRID, (1.0, 0.3, 1.0, 0.5), ((0, 0.5), (0, 0.9), (5, 0.9), (65, 1.0))):
        got = eng.debug_sched_cut_rows(x, mark, b, u, ratio=0.5, seed=seed, step_id=step_id, temperature=tau, top_k=cut[0], top_p=cut[1],
                                       pad_value=float('nan'))
        coin, u2 = sch.coins(seed, step_id, b, u)
        replaced = (u >= 1) & (gold >= 0) & (coin < np.float32(0.5))
        assert np.array_equal(got != mark, replaced) and 0 < replaced.sum() < len(x)
        device = eng.debug_sample_cut_rows(x, tau, cut[0], cut[1], u=u2)[0]
        assert np.array_equal(got[replaced], device[replaced]), (V, cut)            # device against device: exactly
        d64, d32 = cu.draw_rows(x, u2, tau, cut), cu.draw_rows(x, u2, tau, cut, np.float32)
        out = cu.left_out(u2, d64, d32, cu.KERNEL_FLOOR)[0]
        assert np.array_equal(got[replaced & ~out], d64['idx'][replaced & ~out]), (V, cut)
        left += int((out & replaced).sum()); n += int(replaced.sum())
        # the cut (0, 1.0) is the mix kernel without one
        plain = eng.debug_sched_rows(x, mark, b, u, ratio=0.5, seed=seed, step_id=step_id, pick='sample', temperature=tau, pad_value=float('nan'))
        assert np.array_equal(eng.debug_sched_cut_rows(x, mark, b, u, ratio=0.5, seed=seed, step_id=step_id, temperature=tau, pad_value=float('nan')), plain)
    assert left <= sch.LEFT_OUT_CAP * n, (left, n)


def _session(case, deterministic=0, persistent=1):
    from cor_asv_ann_amd.engine import HipEngine
    name, d, W, V, lens, keep, flags, with_masks = case
    eng = HipEngine(d, W, V, **{f: True for f in flags})
    eng.set_weights(sch.build(case)[1])
    eng.set_option('persistent', persistent)
    eng.set_option('deterministic', deterministic)
    eng.train_begin()
    return eng


def _sampled(case, mode=2, deterministic=0, persistent=1, **kw):
    eng = _session(case, deterministic, persistent)
    try:
        kw = dict(dict(seed=sch.SEED, step_id=sch.STEP_ID), **kw)
        loss, norm, mixes = eng.train_step_sampled(*sch.build(case)[3], mode=mode, **kw)
        grads = eng.train_gradients()
        eng.train_end()
        return float(loss), float(norm), mixes, grads
    finally:
        eng.close()


def _equal(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize('cut', [(0, 0.5), (5, 1.0)])
def test_sampled_step_under_a_cut_follows_the_oracle(cut):
    case = sch.STEP_CASES[0]
    gold = sch.build(case)[3][2]
    U = gold.shape[1]
    tau = 0.7
    kw = dict(ratio=0.5, pick='sample', temperature=tau, top_k=cut[0], top_p=cut[1])
    seq, seq_out = gold.copy(), np.zeros(gold.shape, bool)          # the sequential procedure on the float64 oracle
    for u in range(1, U):
        mix, lo = cu.sched_next_mix(case, seq, gold, 0.5, tau, cut)
        seq[:, u], seq_out[:, u] = mix[:, u], lo[:, u]
    for passes in (1, 2):
        loss, norm, mixes, _ = _sampled(case, passes=passes, persistent=1, **kw)
        per_step = _sampled(case, passes=passes, persistent=0, **kw)
        assert np.array_equal(per_step[2], mixes), passes         # the per-step and the persistent form: the same mix
        assert mixes.shape == (passes,) + gold.shape and (mixes[-1] != gold).any() and np.isfinite(loss)
        cur = gold
        for p in range(passes):
            want, out = cu.sched_next_mix(case, cur, gold, 0.5, tau, cut)
            print('%s cut %r pass %d of %d: %d of %d positions left out, %d replaced' % (case[0], cut, p + 1, passes, out.sum(), out.size, (mixes[p] != gold).sum()))
            assert out.sum() <= sch.LEFT_OUT_CAP * out.size
            assert np.array_equal(mixes[p][~out], want[~out]), (cut, p, mixes[p], want)
            cur = mixes[p]
        ahead = slice(0, passes + 1)                                # the first positions are the sequential procedure's
        sure = ~seq_out[:, ahead].any(axis=1)                       # (rows without a left-out draw on the way)
        assert sure.any() and np.array_equal(mixes[-1][sure][:, ahead], seq[sure][:, ahead]), (cut, passes)


def test_sampled_step_cut_contract():
    from cor_asv_ann_amd._native import NativeError
    from cor_asv_ann_amd import _native as nv
    case = sch.STEP_CASES[0]
    batch = sch.build(case)[3]
    # the cut (0, 1.0) through the _cut entry: casv_train_step_sampled's bits
    a = _sampled(case, deterministic=1, ratio=0.5, passes=2, pick='sample', temperature=0.7)
    eng = _session(case, deterministic=1)
    try:
        p = eng._sched_params(sch.SEED, sch.STEP_ID, 0.5, 'sample', 2, 0.7)
        idx = np.ascontiguousarray(batch[0][:, :, None])
        B, T, A = idx.shape
        U = batch[2].shape[1]
        mixes = np.empty((2, B, U), np.int32)
        loss, norm = ctypes.c_double(), ctypes.c_double()

        def call(cut, params=p, out=mixes, mode=2):
            return eng.lib.casv_train_step_sampled_cut(eng.handle, mode, B, T, U, A, nv.ptr(idx), None, nv.ptr(batch[2]), nv.ptr(batch[3]),
                                                       nv.ptr(batch[4]), None, None, None, ctypes.byref(params), None if cut is None else ctypes.byref(cut),
                                                       None if out is None else nv.ptr(out), ctypes.byref(loss), ctypes.byref(norm))
        assert call(nv.SampleCut(0, 1.0)) == 0
        assert loss.value == a[0] and norm.value == a[1] and np.array_equal(mixes, a[2]) and _equal(eng.train_gradients(), a[3])
        # refusals: the session's state stays
        assert eng.train_step(*batch, mode=1)
        before = (eng.train_state(), eng.train_gradients())
        greedy = eng._sched_params(sch.SEED, sch.STEP_ID, 0.5, 'greedy', 2, 0.7)
        for rc in (call(None), call(nv.SampleCut(-1, 1.0)), call(nv.SampleCut(4096, 1.0)), call(nv.SampleCut(0, 0.0)), call(nv.SampleCut(0, -0.1)),
                   call(nv.SampleCut(0, 1.5)), call(nv.SampleCut(0, float('nan'))), call(nv.SampleCut(5, 1.0), greedy), call(nv.SampleCut(0, 0.9), greedy),
                   call(nv.SampleCut(0, 0.9), mode=0), call(nv.SampleCut(0, 0.9), out=None)):
            assert rc == -1
            (m, v, step), grads = eng.train_state(), eng.train_gradients()
            assert step == 1 and _equal(grads, before[1]) and _equal(m, before[0][0]) and _equal(v, before[0][1])
        assert call(nv.SampleCut(0, 1.0), greedy) == 0              # no cut with the greedy pick: allowed
        with pytest.raises(NativeError):
            eng.train_step_sampled(*batch, ratio=0.5, pick='greedy', top_p=0.9)
        with pytest.raises(NativeError):
            eng.debug_sched_cut_rows(np.zeros((2, 12), np.float32), [1, 1], [0, 1], [1, 1], pick='greedy', top_k=3)
        eng.train_end()
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------ d. the facade
def _facade(case, batch_size, seed=None):
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence
    from oracle.decode import OracleModel
    mc = sa.build_model(case)
    s2s = Sequence2Sequence()
    s2s.depth, s2s.width, s2s.batch_size = case[1], case[2], batch_size
    s2s.mapping, s2s.voc_size = OracleModel(mc['cfg'], mc['w']).mapping, case[3]
    s2s.seed = seed
    s2s.configure()
    s2s.set_weights(mc['w'])
    s2s.status = 2
    i_c = s2s.mapping[1]
    return s2s, [''.join(i_c[int(i)] for i in row) for row in mc['idx']]


@pytest.mark.parametrize('kw', [dict(top_p=0.9), dict(top_k=100)], ids=['top_p_0.9', 'top_k_100'])
def test_sample_lines_do_not_move_with_the_batch_size(kw):
    runs = []
    for batch_size in (2, 4, 12):
        s2s, lines = _facade(sa.FACADE_CASE, batch_size)
        runs.append(s2s.sample_lines(lines, n=2, seed=5, temperature=0.9, **kw)[:4])
        s2s.engine.close()
    assert runs[0] == runs[1] == runs[2]
    s2s, lines = _facade(sa.FACADE_CASE, 4)
    plain = s2s.sample_lines(lines, n=2, seed=5, temperature=0.9)[:4]
    if 'top_p' in kw:
        assert plain != runs[0]                                   # the nucleus cuts something on these near-flat models
    else:
        assert plain == runs[0]                                   # top_k = 100 >= V - 1 = 39: all candidates, the same lines
    s2s.engine.close()


def test_train_with_a_cut_checkpoints_and_resumes(tmp_path, monkeypatch):
    from cor_asv_ann_amd import keras_h5
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence
    from cor_asv_ann_amd.synthetic import make_lines
    lines, _ = make_lines(160, 9, 5, voc_size=24)             # (a fifth of them validate: two batches of 16)
    corpus = str(tmp_path / 'train.tsv')
    with open(corpus, 'w') as f:
        f.write(''.join('%s\t%s\n' % (l[:-1], l[:-1]) for l in lines))
    monkeypatch.chdir(tmp_path)

    def model(epochs):
        s2s = Sequence2Sequence(progbars=False)
        s2s.depth, s2s.width, s2s.batch_size, s2s.epochs = 1, 32, 16, epochs
        s2s.seed, s2s.deterministic, s2s.checkpoint_training_state = 11, True, True
        s2s.configure()
        return s2s
    good = dict(sample_schedule=0.5, sample_pick='sample', sample_top_p=0.9)
    first = model(1)
    first.train([corpus], **good)
    assert len(first.history) == 1 and np.isfinite(first.history[0]['loss'])
    (ck,) = glob.glob('model.ckpt.weights-01-*.h5')
    state = keras_h5.read_training_state(ck)['sample']
    assert state['top_k'] == 0 and state['top_p'] == 0.9 and state['pick'] == 'sample'
    for change in (dict(sample_top_p=0.8), dict(sample_top_p=1.0), dict(sample_top_k=5)):
        with pytest.raises(ValueError, match='differs'):
            model(2).train([corpus], resume=ck, **dict(good, **change))
    resumed = model(2)
    resumed.train([corpus], resume=ck, **good)
    assert len(resumed.history) == 2 and np.isfinite(resumed.history[1]['loss'])
