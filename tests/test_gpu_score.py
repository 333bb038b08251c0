"""score_targets on the device (csrc/score.hip: casv_score_targets; csrc/train_kernels.hip: score_rows_kernel): the head alone against
float64, the model against the oracle in every launch form, what the call leaves of the handle's state, the independence of a
batch's rows, the give-up path and the facade's score_lines.  Cases, references and bounds: tests/score_cases.py, held on the CPU by
tests/test_score_cases.py.  Runs with and without CASV_POISON=1 (fresh device buffers hold NaN / -1)."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import score_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = {'fused': (('persistent', -1),), 'stepwise': (('persistent', 0),), 'deterministic': (('deterministic', 1),)}


def _engine(c, form='fused'):
    from cor_asv_ann_amd.engine import HipEngine
    mc = sc.model_case(c)
    eng = HipEngine(c[0], c[1], c[2], **mc['flags'])
    eng.set_weights(mc['w'])
    for k, v in FORMS[form]:
        eng.set_option(k, v)
    return eng, mc


def _score(eng, mc, **kw):
    return eng.score_targets(mc['enc_idx'], mc['enc_val'], mc['din'], kw.pop('dout', mc['dout']), **kw)


def _same(a, b):
    """Bit for bit, a NaN equal to a NaN."""
    return all(np.array_equal(x, y, equal_nan=x.dtype.kind == 'f') for x, y in zip(a, b))


def _close_logp(a, b, p):
    """The bound of (b) between two device results: 2e-4 + 2e-6 / p around either."""
    return np.abs(a - b) <= 2 * (2e-4 + 2e-6 / np.maximum(p, 1e-300))


# ------------------------------------------------------------------------------------------------------------------ a. the head alone
@pytest.fixture(scope='module')
def head_engine():
    from cor_asv_ann_amd.engine import HipEngine
    eng = HipEngine(1, 32, 40)
    yield eng
    eng.close()


_head_worst = {}


@pytest.mark.parametrize('V', sc.HEAD_V)
def test_head_against_float64(head_engine, V):
    """logp within 4 E_np units of the float64 head -- E_np the float32-numpy head's own error (tests/test_score_cases.py), the
    margin of 4 for the device's expf / logf and its wave-tree sum; best and rank exact; no output moves with the padding columns."""
    bound = 4 * sc.e_np()
    for s in sc.HEAD_SCALES:
        x, t = sc.head_case(V, s)
        want = sc.head64(x, t)
        first = None
        for pad in sc.PADS:
            got = head_engine.debug_score_rows(x, t, pad)
            ratio = float(sc.units(got[0], want[0]).max()) / bound
            print('V=%d s=%g pad=%r: %.3f of the bound' % (V, s, pad, ratio))
            _head_worst[(V, s)] = max(_head_worst.get((V, s), 0.0), ratio)
            assert ratio <= 1
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
            assert (got[0][t < 0] == 0).all() and (got[2][t < 0] == -1).all()
            first = first or got
            assert _same(got, first), pad
        if s == 80.0 and V >= 63:
            assert want[0].min() < -100
    if len(_head_worst) == len(sc.HEAD_V) * len(sc.HEAD_SCALES):        # the last V: the record of the run
        try:
            f = open(os.path.join(ROOT, 'profiles', 'score_head_error.txt'), 'w')
        except OSError:                     # (a read-only checkout: the assertions above are the test, the file is the record)
            return
        with f:
            f.write('scoring head on the device against float64: largest |logp - logp64| as a fraction of the bound\n'
                    '4 x E_np x 2^-24 (|logp64| + 1), E_np = %.3f (the float32-numpy head), R = %d rows per case, four padding values\n'
                    % (sc.e_np(), sc.HEAD_R))
            for (v, s), r in sorted(_head_worst.items()):
                f.write('V=%-5d s=%-3g %.3f\n' % (v, s, r))
            f.write('largest: %.3f\n' % max(_head_worst.values()))


def test_head_on_constructed_rows(head_engine):
    bound = 4 * sc.e_np()
    for name, x, t in sc.constructed_rows():
        want = sc.head64(x[None], [t])
        for pad in sc.PADS:
            got = head_engine.debug_score_rows(x[None], np.array([t], np.int32), pad)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (name, pad, got, want)
            u = sc.units_or_inf(got[0], want[0])
            assert u.max() <= bound, (name, pad, got[0], want[0])
    got = head_engine.debug_score_rows(np.full((1, 40), 1.5, np.float32), np.array([7], np.int32))
    assert got[1][0] == 0 and got[2][0] == 0 and abs(float(got[0][0]) + np.log(40)) <= bound * sc.UNIT * (np.log(40) + 1)


# ------------------------------------------------------------------------------------------------------------------ b. the model
def _check_against_oracle(c, mc, o, got, aligned=True):
    logp, best, rank, nll, count, align = got
    dout = mc['dout']
    scored = dout >= 0
    p = np.exp(logp.astype(np.float64))
    err32 = np.abs(p - o['pt32'])[scored] - (2e-4 * o['pt32'][scored] + 2e-6)
    err64 = np.abs(logp - np.log(o['pt64']))[scored] - (2e-4 + 2e-6 / o['pt64'][scored])
    print('%s: exp(logp) vs fp32 %.3f, logp vs fp64 %.3f of the bounds' % (
        sc.case_id(c), (np.abs(p - o['pt32'])[scored] / (2e-4 * o['pt32'][scored] + 2e-6)).max(),
        (np.abs(logp - np.log(o['pt64']))[scored] / (2e-4 + 2e-6 / o['pt64'][scored])).max()))
    assert (err32 <= 0).all() and (err64 <= 0).all()
    assert (logp[~scored] == 0).all() and (rank[~scored] == -1).all()
    keep = o['agree']
    assert keep.mean() >= 0.98
    assert np.array_equal(best[keep], o['best64'][keep]) and np.array_equal(rank[keep], o['rank64'][keep])
    assert np.array_equal(count, scored.sum(axis=1))
    want_nll, _ = sc.nll_of(logp, dout)
    assert np.array_equal(nll.view(np.int64), want_nll.view(np.int64))
    if aligned and o['rows64'] is not None:
        assert align is not None and np.allclose(align, o['rows64'], rtol=2e-4, atol=2e-6)


@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('c', sc.MODEL_CASES, ids=sc.IDS)
def test_score_targets_matches_oracle(c, form):
    eng, mc = _engine(c, form)
    o = sc.oracles(c)
    got = _score(eng, mc, want_align=True)
    _check_against_oracle(c, mc, o, got)
    logp, best, rank, nll, count, align = got
    B, U = mc['dout'].shape
    T = mc['enc_in'].shape[1]
    # the window form: the dense rows bit for bit inside the window, and the dense rows are 0 outside
    sparse = _score(eng, mc, want_align='sparse')
    lo, w = sparse[5]
    K = w.shape[2]
    assert lo.shape == (B, U) and K == 11
    if form == 'deterministic':
        assert _same(sparse[:5], got[:5])
    for b in range(B):
        for u in range(U):
            inside = np.zeros(T, bool)
            assert lo[b, u] >= 0                                            # (no window falls off these lines)
            n = min(K, T - lo[b, u])
            inside[lo[b, u]:lo[b, u] + n] = True
            if form == 'deterministic':
                assert np.array_equal(align[b, u, inside], w[b, u, :n])
            else:
                assert np.allclose(align[b, u, inside], w[b, u, :n], rtol=4e-4, atol=4e-6)     # (two calls: their sums' order may differ)
            assert (w[b, u, n:] == 0).all() and (align[b, u, ~inside] == 0).all()
    dense_again = _score(eng, mc, want_align=True)
    lo2, w2 = np.empty_like(lo), np.empty_like(w)
    from cor_asv_ann_amd import _native as nv
    nv.check(eng.lib.casv_score_get_alignments_sparse(eng.handle, K, nv.ptr(lo2), nv.ptr(w2)))
    for b in range(B):
        for u in range(U):
            n = min(K, T - lo2[b, u])
            assert np.array_equal(dense_again[5][b, u, lo2[b, u]:lo2[b, u] + n], w2[b, u, :n])         # the SAME call: bit for bit
    # targets the model finds best: dec_out = the first call's best, dec_in unchanged
    top = _score(eng, mc, dout=best)
    assert (top[2] == 0).all() and np.array_equal(top[1], best)
    scored = mc['dout'] >= 0
    assert (top[0][scored] >= logp[scored] - 1e-3).all()
    agreed = scored & (rank == 0)
    if form == 'deterministic':
        assert np.array_equal(top[0][agreed], logp[agreed]) and (top[0][scored] >= logp[scored]).all()
    else:
        assert _close_logp(top[0][agreed], logp[agreed], np.exp(logp[agreed].astype(np.float64))).all()
    eng.close()


@pytest.mark.parametrize('c', sc.MODEL_CASES, ids=sc.IDS)
def test_relation_to_the_mode_0_loss(c):
    """Inside a session: the mode-0 loss times the number of weighted positions is the sum of -log(clip(exp(logp))), and the
    scoring call takes the persistent launches the mode-0 step takes."""
    eng, mc = _engine(c)
    eng.train_begin()
    loss, _ = eng.train_step(mc['enc_idx'], mc['enc_val'], mc['din'], mc['dout'], mc['wts'], None, mode=0)
    launches = eng.stat('train_persistent_launches')
    got = _score(eng, mc)
    assert eng.stat('train_persistent_launches') == launches
    _check_against_oracle(c, mc, sc.oracles(c), got, aligned=False)
    scored = mc['dout'] >= 0
    p = np.clip(np.exp(got[0].astype(np.float64)), 1e-7, 1 - 1e-7)
    total = -np.log(p[scored]).sum()
    assert abs(loss * scored.sum() - total) <= 2e-5 * total
    if c == sc.BLOCK_CASE:
        assert launches >= 1                # (this case's recurrences have persistent forms)
    eng.train_end()
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ c. state
def _get_step(eng):
    from cor_asv_ann_amd import _native as nv
    step = ctypes.c_int64()
    nv.check(eng.lib.casv_train_get_step(eng.handle, ctypes.byref(step)))
    return step.value


CASE_C = sc.MODEL_CASES[2]


def test_outside_a_session_the_call_leaves_no_session():
    from cor_asv_ann_amd._native import NativeError
    eng, mc = _engine(CASE_C, 'deterministic')
    with pytest.raises(NativeError) as e:
        _get_step(eng)
    assert e.value.code == -2
    first = _score(eng, mc, want_align=True)
    with pytest.raises(NativeError) as e:
        _get_step(eng)
    assert e.value.code == -2
    assert _same(_score(eng, mc, want_align=True), first)          # the kept state scores the same bits
    eng.score_release()
    eng.score_release()                                             # allowed twice
    assert _same(_score(eng, mc, want_align=True), first)
    # other weights: the state is rebuilt, the results are a fresh handle's
    w2 = {k: (v * np.float32(0.9)) for k, v in mc['w'].items()}
    eng.set_weights(w2)
    got = _score(eng, mc, want_align=True)
    from cor_asv_ann_amd.engine import HipEngine
    fresh = HipEngine(CASE_C[0], CASE_C[1], CASE_C[2])
    fresh.set_weights(w2)
    fresh.set_option('deterministic', 1)
    want = _score(fresh, mc, want_align=True)
    fresh.close()
    assert _same(got, want) and not _same(got, first)
    eng.train_begin()                                               # works afterwards
    assert _get_step(eng) == 0
    assert _same(_score(eng, mc, want_align=True), want)           # ... and the session scores its own (the same) weights
    eng.train_end()
    eng.close()


def test_inside_a_session_the_call_changes_nothing():
    def run(score):
        eng, mc = _engine(CASE_C, 'deterministic')
        eng.train_begin()
        args = (mc['enc_idx'], mc['enc_val'], mc['din'], mc['dout'], mc['wts'], None)
        eng.train_step(*args, mode=1)
        before = eng.train_state()
        scored = None
        if score:
            scored = _score(eng, mc, want_align=True)
            after = eng.train_state()
            assert after[2] == before[2] == 1
            for name in ('E', 'dec%d_K' % CASE_C[0]):
                assert np.array_equal(after[0][name], before[0][name]) and np.array_equal(after[1][name], before[1][name])
        out = eng.train_step(*args, mode=1)
        w = eng.train_weights()
        eng.train_end()
        eng.close()
        return out, w, scored
    out_a, w_a, scored = run(True)
    out_b, w_b, _ = run(False)
    assert out_a == out_b and all(np.array_equal(w_a[k], w_b[k]) for k in w_a)
    assert np.isfinite(scored[0]).all()


def test_a_decode_after_a_scoring_call_equals_a_fresh_handles():
    eng, mc = _engine(CASE_C)
    _score(eng, mc)
    eng.encode(mc['enc_idx'], None)
    got = eng.decode_greedy(mode=0)
    from cor_asv_ann_amd.engine import HipEngine
    fresh = HipEngine(CASE_C[0], CASE_C[1], CASE_C[2])
    fresh.set_weights(mc['w'])
    fresh.encode(mc['enc_idx'], None)
    want = fresh.decode_greedy(mode=0)
    assert _same(got[:3], want[:3])
    fresh.close()
    eng.close()


def test_out_of_range_indices_are_refused_before_any_launch():
    from cor_asv_ann_amd._native import NativeError
    eng, mc = _engine(CASE_C)
    V = CASE_C[2]
    before = eng.stat('train_persistent_launches')
    for which, value in (('dout', V), ('dout', -2), ('din', V), ('din', -2), ('dout', 2 ** 31 - 1)):
        din, dout = mc['din'].copy(), mc['dout'].copy()
        (din if which == 'din' else dout)[2, 3] = value
        with pytest.raises(NativeError) as e:
            eng.score_targets(mc['enc_idx'], None, din, dout)
        assert e.value.code == -1, (which, value)
    with pytest.raises(NativeError) as e:           # nothing was built either: there is no scoring call to take alignments from
        lo, w = np.empty(mc['dout'].shape, np.int32), np.empty(mc['dout'].shape + (11,), np.float32)
        from cor_asv_ann_amd import _native as nv
        nv.check(eng.lib.casv_score_get_alignments_sparse(eng.handle, 11, nv.ptr(lo), nv.ptr(w)))
    assert e.value.code == -2 and eng.stat('train_persistent_launches') == before
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ d. rows are independent
@pytest.mark.parametrize('form', ['deterministic', 'fused'])
def test_rows_are_independent(form):
    """The padded T and U fixed at the array level: line i alone, in the batch of 37 and in the batch reversed."""
    c = sc.BLOCK_CASE
    eng, mc = _engine(c, form)
    full = _score(eng, mc, want_align=True)
    rev = eng.score_targets(mc['enc_idx'][::-1], None, mc['din'][::-1], mc['dout'][::-1], want_align=True)
    ones = {i: eng.score_targets(mc['enc_idx'][i:i + 1], None, mc['din'][i:i + 1], mc['dout'][i:i + 1], want_align=True) for i in (0, 1, 31, 32, 36)}
    eng.close()
    B = c[3]
    bit_equal = _same([a[::-1] for a in rev], full) and all(_same([a[i:i + 1] for a in full], one) for i, one in ones.items())
    print('rows independent, %s form: bit for bit %s' % (form, bit_equal))
    if form == 'deterministic':
        assert bit_equal
        return
    p = np.exp(full[0].astype(np.float64))
    for other, sel in [(rev, slice(None, None, -1))] + [(one, slice(i, i + 1)) for i, one in ones.items()]:
        sub = [a[sel] for a in full]
        assert _close_logp(other[0], sub[0], p[sel]).all()
        assert np.array_equal(other[1], sub[1]) and np.array_equal(other[2], sub[2]) and np.array_equal(other[4], sub[4])
        assert np.allclose(other[3], sub[3], rtol=0, atol=2 * (2e-4 + 2e-6 / p[sel].min()) * mc['dout'].shape[1])
        assert np.allclose(other[5], sub[5], rtol=4e-4, atol=4e-6)
    assert B == 37


# ------------------------------------------------------------------------------------------------------------------ e. the give-up path
def test_a_forward_recurrence_that_gives_up_is_redone_per_step(capfd):
    c = sc.BLOCK_CASE
    eng, mc = _engine(c, 'stepwise')
    want = _score(eng, mc, want_align=True)
    ups = eng.stat('train_give_ups')
    capfd.readouterr()
    eng.set_option('persistent', 2)
    got = _score(eng, mc, want_align=True)
    assert 'gave up waiting' in capfd.readouterr().err
    assert eng.stat('train_give_ups') == ups + 1 and eng.stat('train_persistent_launches') == 0
    _check_against_oracle(c, mc, sc.oracles(c), got)
    assert _same(got[1:3], want[1:3]) and _close_logp(got[0], want[0], np.exp(want[0].astype(np.float64))).all()
    again = _score(eng, mc, want_align=True)                    # backed off: per step, no message, no further give-up
    assert 'gave up waiting' not in capfd.readouterr().err
    assert eng.stat('train_give_ups') == ups + 1 and eng.stat('train_persistent_launches') == 0
    _check_against_oracle(c, mc, sc.oracles(c), again)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ f. the facade
def test_score_lines_through_the_facade():
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence
    from cor_asv_ann_amd.realign import SparseAlignment
    from cor_asv_ann_amd.training import batch_to_indices
    from oracle import ModelConfig, make_weights, make_lines
    from oracle.decode import OracleModel
    cfg = ModelConfig(depth=2, width=64, voc_size=96)           # tests/golden/d2_w64_v96.npz's model
    weights = make_weights(cfg, emb_scale=12.0)
    s2s = Sequence2Sequence()
    s2s.depth, s2s.width, s2s.batch_size = cfg.depth, cfg.width, 2
    s2s.mapping, s2s.voc_size = OracleModel(cfg, weights).mapping, cfg.voc_size
    s2s.configure()
    s2s.set_weights(weights)
    s2s.status = 2
    sources, _ = make_lines(5, 12, 5, voc_size=96)
    targets, _ = make_lines(5, 10, 6, voc_size=96)
    targets[1] = ''
    targets[3] = targets[3][:4] + '\n'
    logprobs, scores, predictions, ranks, aligns = s2s.score_lines(sources, targets)
    assert [len(x) for x in logprobs] == [len(t) for t in targets] == [len(x) for x in ranks]
    assert (logprobs[1], scores[1], predictions[1], ranks[1], aligns[1]) == ([], 0.0, '', [], []) and aligns == [[]] * 5
    assert all(isinstance(p, str) and len(p) <= len(t) for p, t in zip(predictions, targets))
    eng = s2s._require_engine()
    eng.set_option('deterministic', 1)
    logprobs, scores, predictions, ranks, sparse = s2s.score_lines(sources, targets, alignments=True)
    dense = s2s.score_lines(sources, targets, alignments='dense')[4]
    live = [0, 2, 3, 4]
    for chunk in (live[:2], live[2:]):                          # each chunk: the values of a direct engine call on its arrays
        idx, val, din, dout, _ = batch_to_indices(s2s, [sources[j] for j in chunk], [targets[j] for j in chunk], None)
        logp, best, rank, nll, count, align = eng.score_targets(idx, val, din, dout, want_align=True)
        for i, j in enumerate(chunk):
            k = len(targets[j])
            assert count[i] == k and logprobs[j] == logp[i, :k].tolist() and ranks[j] == rank[i, :k].tolist()
            assert scores[j] == nll[i] / count[i]
            assert predictions[j] == s2s._chars(best[i, :k])
            assert isinstance(sparse[j], SparseAlignment) and len(sparse[j]) == k == len(dense[j])
            assert np.array_equal(np.asarray(dense[j]), align[i, :k]) and np.array_equal(np.asarray(sparse[j]), align[i, :k])
    assert sparse[1] == [] and dense[1] == []
