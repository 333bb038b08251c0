"""score_candidates on the device (csrc/score.hip: casv_score_candidates): N candidate targets per source on one encoder pass against
score_targets on the replicated pairs and against the oracle, in every launch form; the N = 1 call, the order of a source's
candidates, the launch form of the mixed-row pair recurrence, the window form, what the call leaves of the handle's state, the
refusals and the facade.  Cases and references: tests/candidate_cases.py, held on the CPU by tests/test_score_candidates_host.py;
the bounds are tests/test_gpu_score.py's, restated."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import candidate_cases as cc
from tests import score_cases as sc

FORMS = {'fused': (('persistent', -1),), 'stepwise': (('persistent', 0),), 'deterministic': (('deterministic', 1),)}


def _engine(c, form='fused'):
    from cor_asv_ann_amd.engine import HipEngine
    k = cc.case(c)
    eng = HipEngine(c[0], c[1], c[2], **k['flags'])
    eng.set_weights(k['w'])
    for key, v in FORMS[form]:
        eng.set_option(key, v)
    return eng, k


def _cand(eng, k, **kw):
    return eng.score_candidates(k['enc_idx'], k['enc_val'], kw.pop('din', k['din']), kw.pop('dout', k['dout']), **kw)


def _pairs(eng, k, **kw):
    """score_targets on the Be * N replicated pairs at the same T, U, A, its outputs in the candidates call's shapes."""
    got = eng.score_targets(k['rep_idx'], k['rep_val'], k['rep_din'], k['rep_dout'], **kw)
    Be, N = k['Be'], k['N']
    shape = lambda a: a.reshape((Be, N) + a.shape[1:])
    align = got[5]
    if isinstance(align, tuple):
        align = tuple(shape(a) for a in align)
    elif align is not None:
        align = shape(align)
    return tuple(shape(a) for a in got[:5]) + (align,)


def _same(a, b):
    """Bit for bit, a NaN equal to a NaN."""
    return all(x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == 'f') for x, y in zip(a, b))


def _padding_is_zero(k, got):
    logp, best, rank, nll, count, align = got
    if k['N'] >= 2:
        assert (logp[-1, -1] == 0).all() and (rank[-1, -1] == -1).all() and count[-1, -1] == 0
        assert nll[-1, -1] == 0 and not np.signbit(nll[-1, -1])


# ------------------------------------------------------------------------------------------------------------------ 1. the replicated pairs
@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('c', cc.CASES, ids=cc.IDS)
def test_equals_score_targets_on_the_replicated_pairs(c, form):
    """Deterministic: all six outputs bit for bit.  The other forms: two calls whose sums may differ in order (the launcher's K
    split follows M, and M = T * Be here against T * Be * N there) -- the project's two-call bound 2 (2e-4 + 2e-6 / p) on logp, count
    equal, nll the sum of this call's logp bit for bit, the attention rows within rtol 4e-4 / atol 4e-6."""
    eng, k = _engine(c, form)
    got = _cand(eng, k, want_align=True)
    want = _pairs(eng, k, want_align=True)
    eng.close()
    Be, N, T, U = k['Be'], k['N'], k['T'], k['U']
    assert got[0].shape == (Be, N, U) and got[3].shape == (Be, N) and got[5].shape == (Be, N, U, T)
    _padding_is_zero(k, got)
    bit_equal = _same(got, want)
    print('%s %s: bit for bit with the replicated pairs: %s' % (cc.case_id(c), form, bit_equal))
    if form == 'deterministic':
        assert bit_equal
        return
    scored = k['dout'] >= 0
    p = np.exp(want[0].astype(np.float64))
    print('  logp: %.3f of the two-call bound' % (np.abs(got[0] - want[0])[scored] / (2 * (2e-4 + 2e-6 / p[scored]))).max())
    assert (np.abs(got[0] - want[0])[scored] <= 2 * (2e-4 + 2e-6 / p[scored])).all()
    assert (got[0][~scored] == 0).all() and (got[2][~scored] == -1).all()
    assert np.array_equal(got[4], want[4]) and np.array_equal(got[4], scored.sum(axis=2))
    want_nll, _ = sc.nll_of(got[0].reshape(Be * N, U), k['rep_dout'])
    assert np.array_equal(got[3].reshape(-1).view(np.int64), want_nll.view(np.int64))
    assert np.allclose(got[5], want[5], rtol=4e-4, atol=4e-6)


# ------------------------------------------------------------------------------------------------------------------ 2. the oracle
@pytest.mark.parametrize('form', ['fused', 'deterministic'])
@pytest.mark.parametrize('c', cc.CASES, ids=cc.IDS)
def test_matches_the_oracle_on_the_replicated_batch(c, form):
    eng, k = _engine(c, form)
    got = _cand(eng, k, want_align=True)
    eng.close()
    o = cc.oracles(c)
    R, U = k['rep_dout'].shape
    logp, best, rank, nll, count = (a.reshape((R,) + a.shape[2:]) for a in got[:5])
    align = got[5].reshape(R, U, k['T'])
    dout = k['rep_dout']
    scored = dout >= 0
    p = np.exp(logp.astype(np.float64))
    r32 = np.abs(p - o['pt32'])[scored] / (2e-4 * o['pt32'][scored] + 2e-6)
    r64 = np.abs(logp - np.log(o['pt64']))[scored] / (2e-4 + 2e-6 / o['pt64'][scored])
    print('%s %s: exp(logp) vs fp32 %.3f, logp vs fp64 %.3f of the bounds' % (cc.case_id(c), form, r32.max(), r64.max()))
    assert (r32 <= 1).all() and (r64 <= 1).all()
    assert (logp[~scored] == 0).all() and (rank[~scored] == -1).all()
    keep = o['agree']
    assert keep.mean() >= 0.98
    assert np.array_equal(best[keep], o['best64'][keep]) and np.array_equal(rank[keep], o['rank64'][keep])
    assert np.array_equal(count, scored.sum(axis=1))
    want_nll, _ = sc.nll_of(logp, dout)
    assert np.array_equal(nll.view(np.int64), want_nll.view(np.int64))
    if o['rows64'] is not None:             # (residual_connections: the stepped restatement is not the training graph)
        assert np.allclose(align, o['rows64'], rtol=2e-4, atol=2e-6)       # (the padding candidate's rows too: zero input rows on both sides)


# ------------------------------------------------------------------------------------------------------------------ 3. N = 1
@pytest.mark.parametrize('c', [sc.MODEL_CASES[2], sc.BLOCK_CASE], ids=[sc.IDS[2], sc.IDS[4]])
def test_one_candidate_per_source_is_score_targets(c):
    from cor_asv_ann_amd.engine import HipEngine
    mc = sc.model_case(c)
    launches = {}
    for form in ('deterministic', 'fused'):
        eng = HipEngine(c[0], c[1], c[2], **mc['flags'])
        eng.set_weights(mc['w'])
        for key, v in FORMS[form]:
            eng.set_option(key, v)
        want = eng.score_targets(mc['enc_idx'], mc['enc_val'], mc['din'], mc['dout'], want_align=True)
        launches['targets'] = eng.stat('train_persistent_launches')
        got = eng.score_candidates(mc['enc_idx'], mc['enc_val'], mc['din'][:, None], mc['dout'][:, None], want_align=True)
        launches['candidates'] = eng.stat('train_persistent_launches')
        eng.close()
        if form == 'deterministic':
            assert _same([a[:, 0] for a in got], want)
            assert launches == {'targets': 0, 'candidates': 0}
        else:
            assert launches['candidates'] == launches['targets']
            if c == sc.BLOCK_CASE:
                assert launches['targets'] >= 1


# ------------------------------------------------------------------------------------------------------------------ 4. candidate order
def test_permuting_a_sources_candidates_permutes_its_results():
    c = cc.CASES[3]                         # 3 sources x 11 candidates
    eng, k = _engine(c, 'deterministic')
    first = _cand(eng, k, want_align=True)
    perm = np.random.default_rng(5).permutation(k['N'])
    assert not np.array_equal(perm, np.arange(k['N']))
    din, dout = k['din'].copy(), k['dout'].copy()
    din[1], dout[1] = din[1][perm], dout[1][perm]
    got = _cand(eng, k, din=din, dout=dout, want_align=True)
    eng.close()
    want = [a.copy() for a in first]
    for a in want:
        a[1] = a[1][perm]
    assert _same(got, want) and not _same(got, first)


# ------------------------------------------------------------------------------------------------------------------ 5. launch form
@pytest.mark.parametrize('c', cc.PLAIN, ids=[cc.case_id(c) for c in cc.PLAIN])
def test_the_mixed_row_pair_goes_persistent(c):
    """The call takes the persistent launches score_targets takes on the replicated batch (the same R): the pair of an encoder
    layer of Be rows and a decoder layer of Be * N rows did not fall back to the per-step launches."""
    eng, k = _engine(c, 'fused')
    _pairs(eng, k)
    want = eng.stat('train_persistent_launches')
    _cand(eng, k)
    got = eng.stat('train_persistent_launches')
    eng.close()
    print('%s: %d persistent launches' % (cc.case_id(c), got))
    assert got == want
    if c[1] % 32 == 0:
        assert got >= 1                     # (every multiple of 32 has a persistent pair recurrence)


# ------------------------------------------------------------------------------------------------------------------ 6. window form
@pytest.mark.parametrize('c', [cc.CASES[3], cc.CASES[4]], ids=[cc.IDS[3], cc.IDS[4]])
def test_window_form_after_a_call(c):
    from cor_asv_ann_amd import _native as nv
    eng, k = _engine(c, 'fused')
    Be, N, T, U = k['Be'], k['N'], k['T'], k['U']
    dense = _cand(eng, k, want_align=True)[5]
    K = 11
    lo, w = np.empty((Be, N, U), np.int32), np.empty((Be, N, U, K), np.float32)
    nv.check(eng.lib.casv_score_get_alignments_sparse(eng.handle, K, nv.ptr(lo), nv.ptr(w)))     # the SAME call's rows: bit for bit
    sparse = _cand(eng, k, want_align='sparse')[5]
    eng.close()
    assert sparse[0].shape == (Be, N, U) and sparse[1].shape == (Be, N, U, K)
    assert np.array_equal(sparse[0], lo)
    assert (lo >= 0).all()                                  # (no window falls off these lines)
    for b in range(Be):
        for n in range(N):
            for u in range(U):
                inside = np.zeros(T, bool)
                cnt = min(K, T - lo[b, n, u])
                inside[lo[b, n, u]:lo[b, n, u] + cnt] = True
                assert np.array_equal(dense[b, n, u, inside], w[b, n, u, :cnt])
                assert (w[b, n, u, cnt:] == 0).all() and (dense[b, n, u, ~inside] == 0).all()


# ------------------------------------------------------------------------------------------------------------------ 7. state
def _get_step(eng):
    from cor_asv_ann_amd import _native as nv
    step = ctypes.c_int64()
    nv.check(eng.lib.casv_train_get_step(eng.handle, ctypes.byref(step)))
    return step.value


CASE_S = cc.CASES[9]                        # depth 4, residual + bridge, 3 x 4


def test_inside_a_session_the_call_changes_nothing():
    def run(score):
        eng, k = _engine(CASE_S, 'deterministic')
        eng.train_begin()
        args = (k['rep_idx'], k['rep_val'], k['rep_din'], k['rep_dout'], k['wts'], None)
        eng.train_step(*args, mode=1)
        before = eng.train_state()
        scored = None
        if score:
            scored = _cand(eng, k, want_align=True)
            after = eng.train_state()
            assert after[2] == before[2] == 1 and _get_step(eng) == 1
            for name in ('E', 'dec%d_K' % CASE_S[0]):
                assert np.array_equal(after[0][name], before[0][name]) and np.array_equal(after[1][name], before[1][name])
        out = eng.train_step(*args, mode=1)
        w = eng.train_weights()
        eng.train_end()
        eng.close()
        return out, w, scored
    out_a, w_a, scored = run(True)
    out_b, w_b, _ = run(False)
    assert out_a == out_b and all(np.array_equal(w_a[name], w_b[name]) for name in w_a)
    assert np.isfinite(scored[0]).all()


def test_outside_a_session_the_call_leaves_no_session_and_a_decode_is_a_fresh_handles():
    from cor_asv_ann_amd._native import NativeError
    from cor_asv_ann_amd.engine import HipEngine
    c = cc.CASES[2]
    eng, k = _engine(c)
    _cand(eng, k)
    with pytest.raises(NativeError) as e:
        _get_step(eng)
    assert e.value.code == -2
    eng.encode(k['enc_idx'], None)
    got = eng.decode_greedy(mode=0)
    fresh = HipEngine(c[0], c[1], c[2])
    fresh.set_weights(k['w'])
    fresh.encode(k['enc_idx'], None)
    want = fresh.decode_greedy(mode=0)
    assert _same(got[:3], want[:3])
    fresh.close()
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals():
    from cor_asv_ann_amd import _native as nv
    from cor_asv_ann_amd._native import NativeError
    c = cc.CASES[2]
    eng, k = _engine(c)
    Be, N, T, U = k['Be'], k['N'], k['T'], k['U']
    before = eng.stat('train_persistent_launches')
    out = (np.empty((Be, N, U), np.float32), np.empty((Be, N, U), np.int32), np.empty((Be, N, U), np.int32),
           np.empty((Be, N), np.float64), np.empty((Be, N), np.int32))
    idx = np.ascontiguousarray(k['enc_idx'][:, :, None])
    with pytest.raises(NativeError) as e:                   # N = 0
        nv.check(eng.lib.casv_score_candidates(eng.handle, Be, 0, T, U, 1, nv.ptr(idx), None, nv.ptr(k['din']), nv.ptr(k['dout']),
                                               *[nv.ptr(a) for a in out], None))
    assert e.value.code == -1
    for which, value in (('dout', c[2]), ('dout', -2), ('din', c[2]), ('din', -2)):         # the last candidate of the last source
        din, dout = k['din'].copy(), k['dout'].copy()
        (din if which == 'din' else dout)[-1, -1, -1] = value
        with pytest.raises(NativeError) as e:
            eng.score_candidates(k['enc_idx'], None, din, dout)
        assert e.value.code == -1, (which, value)
    with pytest.raises(NativeError) as e:                   # nothing was launched or built: no scoring call to take alignments from
        lo, w = np.empty((Be, N, U), np.int32), np.empty((Be, N, U, 11), np.float32)
        nv.check(eng.lib.casv_score_get_alignments_sparse(eng.handle, 11, nv.ptr(lo), nv.ptr(w)))
    assert e.value.code == -2 and eng.stat('train_persistent_launches') == before
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 9. the facade
def test_score_candidates_through_the_facade():
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence
    from cor_asv_ann_amd.realign import SparseAlignment
    from oracle import ModelConfig, make_weights, make_lines
    from oracle.decode import OracleModel
    cfg = ModelConfig(depth=2, width=64, voc_size=96)
    weights = make_weights(cfg, emb_scale=12.0)
    s2s = Sequence2Sequence()
    s2s.depth, s2s.width, s2s.batch_size = cfg.depth, cfg.width, 8
    s2s.mapping, s2s.voc_size = OracleModel(cfg, weights).mapping, cfg.voc_size
    s2s.configure()
    s2s.set_weights(weights)
    s2s.status = 2
    s2s._require_engine().set_option('deterministic', 1)
    sources, _ = make_lines(3, 12, 5, voc_size=96)
    pool, _ = make_lines(7, 10, 6, voc_size=96)
    pool[4] = pool[4][:4] + '\n'
    # equal padded lengths on both sides: 2 sources x 3 candidates in one chunk, against score_lines on the six pairs in one chunk
    cands = [pool[0:3], pool[3:6]]
    got = s2s.score_candidates(sources[:2], cands, alignments='dense')
    want = s2s.score_lines([sources[0]] * 3 + [sources[1]] * 3, pool[:6], alignments='dense')
    flat = [[x for per_source in g for x in per_source] for g in got]
    assert all(len(f) == 6 for f in flat)
    assert flat[0] == want[0] and flat[1] == want[1] and flat[2] == want[2] and flat[3] == want[3]      # logprobs, scores, predictions, ranks
    for a, b in zip(flat[4], want[4]):
        assert len(a) == len(b) > 0 and all(np.array_equal(x, y) for x, y in zip(a, b))
    assert [len(x) for x in got[0][1]] == [len(t) for t in cands[1]] and len(got[0][1][1]) == 5
    # ragged lists, an empty source, an empty candidate, a source without candidates: only their own entries
    ragged = [pool[0:1], [pool[1], '', pool[2]], []]
    logprobs, scores, predictions, ranks, aligns = s2s.score_candidates(sources, ragged, alignments=True)
    assert [len(x) for x in logprobs] == [1, 3, 0] == [len(x) for x in aligns]
    assert (logprobs[1][1], scores[1][1], predictions[1][1], ranks[1][1], aligns[1][1]) == ([], 0.0, '', [], [])
    for j, i in ((0, 0), (1, 0), (1, 2)):
        n = len(ragged[j][i])
        assert len(logprobs[j][i]) == n == len(ranks[j][i]) and isinstance(aligns[j][i], SparseAlignment) and len(aligns[j][i]) == n
        acc = 0.0
        for x in logprobs[j][i]:
            acc += -x
        assert scores[j][i] == acc / n
        assert isinstance(predictions[j][i], str) and len(predictions[j][i]) <= n
