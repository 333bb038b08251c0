"""score_alternatives on the device (csrc/train_kernels.hip: score_alternatives_kernel; csrc/score.hip: casv_score_get_alternatives):
the kernel alone against float64 and against the scoring head's bits, the model against the fp64 oracle in every launch form, the
retrieval behind score_candidates and inside a training session, its state and argument errors, and the facade.  Cases, references
and bounds: tests/alternative_cases.py, held on the CPU by tests/test_alternative_cases.py.  Runs with and without CASV_POISON=1."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import alternative_cases as ac
from tests import candidate_cases as cc
from tests import score_cases as sc

FORMS = {'fused': (('persistent', -1),), 'stepwise': (('persistent', 0),), 'deterministic': (('deterministic', 1),)}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same(a, b):
    """Bit for bit."""
    return all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


def _engine(c, form='fused', mc=None):
    from cor_asv_ann_amd.engine import HipEngine
    mc = mc or sc.model_case(c)
    eng = HipEngine(c[0], c[1], c[2], **mc['flags'])
    eng.set_weights(mc['w'])
    for k, v in FORMS[form]:
        eng.set_option(k, v)
    return eng, mc


def _score(eng, mc):
    return eng.score_targets(mc['enc_idx'], mc['enc_val'], mc['din'], mc['dout'])


# ------------------------------------------------------------------------------------------------------------------ a. the kernel alone
@pytest.fixture(scope='module')
def head_engine():
    from cor_asv_ann_amd.engine import HipEngine
    eng = HipEngine(1, 32, 40)
    yield eng
    eng.close()


def _check_rows(eng, x, K, name):
    """One batch of rows under the four padding values: the comparator, the padding, the head's bits."""
    want = ac.alts64(x, K)
    first = None
    for pad in sc.PADS:
        got = eng.debug_alternatives_rows(x, K, pad)
        assert got[0].shape == got[1].shape == (len(x), K) and got[2].shape == (len(x),)
        ok, lp, h = ac.compare(got, x, K, want)
        print('%s K=%d pad=%r: alt_logp %.3f, entropy %.3f of the bounds' % (name, K, pad, lp, h))
        assert ok, (name, K, pad, got[0], want[0])
        assert lp <= 1 and h <= 1, (name, K, pad)
        first = first or got
        assert _same(got, first), (name, K, pad)
    got = first
    invalid = want[0][:, 0] < 0             # NaN, -inf and -1 exactly where the definition puts them
    assert (got[0][invalid] == -1).all() and np.isnan(got[1][invalid]).all() and np.isnan(got[2][invalid]).all()
    assert (got[0][~invalid] >= 0).all() and not np.isnan(got[1][~invalid]).any() and np.isfinite(got[2][~invalid]).all()
    assert np.array_equal(got[1] == -np.inf, want[1] == -np.inf)
    for j in range(K):                      # alt_logp[j]: the bits of the head's logp for alt_idx[j] as target on the same row
        head = eng.debug_score_rows(x, got[0][:, j])
        assert np.array_equal(_bits(head[0][~invalid]), _bits(got[1][~invalid, j])), (name, K, j)
        assert (head[2][~invalid] <= j).all() and np.isnan(head[0][invalid]).all()      # (at most j entries above it)
    return got


@pytest.mark.parametrize('V', sc.HEAD_V)
def test_kernel_against_float64_and_the_head(head_engine, V):
    """alt_idx exact, alt_logp within 4 E_np units of float64 and the head's bits, entropy within 4 E_H units -- E_np and E_H the
    float32-numpy restatement's own errors, the margin of 4 for the device's expf / logf and its wave-tree sums; no output bit moves
    with the padding columns."""
    for s in sc.HEAD_SCALES:
        x, _ = sc.head_case(V, s)
        for K in ac.head_ks(V):
            _check_rows(head_engine, x, K, 'V=%d s=%g' % (V, s))


def test_kernel_on_constructed_rows(head_engine):
    for name, x, K in ac.constructed_rows():
        _check_rows(head_engine, x[None], K, name)


def test_kernel_with_more_rows_than_one_pass_of_the_grid(head_engine):
    """More rows than the grid's 2048 workgroups x 4 waves take at once, each its own: the grid-stride loop and the wave's LDS rows."""
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((8192 + 37, 96)) * 4).astype(np.float32)
    got = head_engine.debug_alternatives_rows(x, 3)
    want = ac.alts64(x, 3)
    assert np.array_equal(got[0], want[0])
    assert sc.units_or_inf(got[1], want[1]).max() <= 4 * sc.e_np() and sc.units_or_inf(got[2], want[2]).max() <= 4 * ac.e_h()


def test_kernel_arguments(head_engine):
    from cor_asv_ann_amd._native import NativeError
    x = np.zeros((2, 40), np.float32)
    for K in (0, 41, 65, -1):
        with pytest.raises(NativeError) as e:
            head_engine.debug_alternatives_rows(x, K)
        assert e.value.code == -1, K
    with pytest.raises(NativeError) as e:
        head_engine.debug_alternatives_rows(np.zeros((1, 100), np.float32), 65)
    assert e.value.code == -1


# ------------------------------------------------------------------------------------------------------------------ b. the model
def _check_against_scores(alt, scores, dout, K):
    """What ties the lists to score_targets' own outputs of the same call."""
    alt_idx, alt_logp, _ = alt
    logp, best, rank = scores[:3]
    assert np.array_equal(alt_idx[:, :, 0], best)
    for b, u in zip(*np.nonzero((dout >= 0) & (rank < K))):
        r = rank[b, u]
        # x at alt_idx[rank] ties the target's: one value, one logp
        assert _bits(alt_logp[b, u, r:r + 1])[0] == _bits(logp[b, u:u + 1])[0], (b, u)
        tied = (_bits(alt_logp[b, u]) == _bits(logp[b, u:u + 1])[0]).sum() > 1
        assert alt_idx[b, u, r] == dout[b, u] or tied, (b, u)


@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('c', sc.MODEL_CASES, ids=sc.IDS)
def test_alternatives_match_the_oracle(c, form):
    eng, mc = _engine(c, form)
    scores = _score(eng, mc)
    for K in (4, 8):
        alt = eng.score_alternatives(K)
        print(sc.case_id(c), form, end=' ')
        ac.check_model(*alt, ac.model_refs(c, K), K)
        _check_against_scores(alt, scores, mc['dout'], K)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ c. other calls
CAND = cc.CASES[2]


def test_after_score_candidates_the_rows_are_the_candidates():
    """N = 3 with one padding candidate: row b * N + n carries candidate n of source b, the padding candidate's rows are filled
    like any other."""
    assert CAND[4] == 3
    case = cc.case(CAND)
    eng, _ = _engine(CAND[:3], 'deterministic', case)
    scores = eng.score_candidates(case['enc_idx'], case['enc_val'], case['din'], case['dout'])
    Be, N, U = case['dout'].shape
    assert (case['dout'][-1, -1] == -1).all()
    flat = [s.reshape((Be * N,) + s.shape[2:]) for s in scores[:3]]
    for K in (4, 8):
        alt = eng.score_alternatives(K)
        assert alt[0].shape == (Be * N, U, K) and alt[2].shape == (Be * N, U)
        ac.check_model(*alt, ac.refs_of(cc.oracles(CAND), K), K)           # (the oracle ran on the replicated batch: the same rows)
        _check_against_scores(alt, flat, case['rep_dout'], K)
        assert (alt[0][-1] >= 0).all() and np.isfinite(alt[1][-1]).all() and np.isfinite(alt[2][-1]).all()
    eng.close()


def _get_step(eng):
    from cor_asv_ann_amd import _native as nv
    step = ctypes.c_int64()
    nv.check(eng.lib.casv_train_get_step(eng.handle, ctypes.byref(step)))
    return step.value


CASE_C = sc.MODEL_CASES[2]


def test_inside_a_session_a_retrieval_changes_nothing():
    def run(retrieve):
        eng, mc = _engine(CASE_C, 'deterministic')
        eng.train_begin()
        args = (mc['enc_idx'], mc['enc_val'], mc['din'], mc['dout'], mc['wts'], None)
        eng.train_step(*args, mode=1)
        scores = _score(eng, mc)
        alt = None
        if retrieve:
            alt = eng.score_alternatives(8)
            assert _get_step(eng) == 1
            assert _same(eng.score_alternatives(8), alt)
        out = eng.train_step(*args, mode=1)
        steps = _get_step(eng)
        eng.train_end()
        eng.close()
        return out, steps, scores, alt
    out_a, steps_a, scores_a, alt = run(True)
    out_b, steps_b, scores_b, _ = run(False)
    assert out_a == out_b                                           # the loss's bits
    assert steps_a == steps_b == 2
    assert (alt[0] >= 0).all() and np.array_equal(alt[0][:, :, 0], scores_a[1])


def test_state_and_argument_errors():
    from cor_asv_ann_amd._native import NativeError
    from cor_asv_ann_amd import _native as nv
    eng, mc = _engine(CASE_C)
    V = CASE_C[2]
    B, U = mc['dout'].shape

    def raw(K):
        """The entry with buffers of the scoring call's shape, whatever the object knows."""
        i, lp, h = np.empty((B, U, 64), np.int32), np.empty((B, U, 64), np.float32), np.empty((B, U), np.float32)
        nv.check(eng.lib.casv_score_get_alternatives(eng.handle, K, nv.ptr(i), nv.ptr(lp), nv.ptr(h)))

    def refused(call, code):
        with pytest.raises(NativeError) as e:
            call()
        assert e.value.code == code
    refused(lambda: raw(4), -2)                                     # before any scoring call
    refused(lambda: eng.score_alternatives(4), -2)
    _score(eng, mc)
    first = eng.score_alternatives(4)
    for K in (0, 65, V + 1, -3):
        refused(lambda: raw(K), -1)
        refused(lambda: eng.score_alternatives(K), -1)
    assert _same(eng.score_alternatives(4), first)                  # a refused call changed nothing
    idx, lp, h = eng.score_alternatives(4, want_entropy=False)      # entropy may be NULL
    assert h is None and _same((idx, lp), first[:2])
    eng.score_release()
    refused(lambda: raw(4), -2)                                     # after casv_score_release
    _score(eng, mc)
    assert _same(eng.score_alternatives(4), first)
    eng.train_begin()
    _score(eng, mc)
    eng.score_alternatives(4)
    eng.train_step(mc['enc_idx'], mc['enc_val'], mc['din'], mc['dout'], mc['wts'], None, mode=1)
    refused(lambda: raw(4), -2)                                     # after a train step
    eng.train_end()
    eng.close()
    c0 = sc.MODEL_CASES[0]                                          # K = V + 1 below 64: a vocabulary of 40
    eng, mc = _engine(c0)
    _score(eng, mc)
    refused(lambda: eng.score_alternatives(c0[2] + 1), -1)
    assert eng.score_alternatives(c0[2])[0].shape[2] == c0[2]       # K = V: every entry, each once
    assert (np.sort(eng.score_alternatives(c0[2])[0], axis=2) == np.arange(c0[2])).all()
    eng.close()


def test_two_retrievals_after_one_scoring_call():
    eng, mc = _engine(sc.BLOCK_CASE)
    scores = _score(eng, mc)
    four = eng.score_alternatives(4)
    eight = eng.score_alternatives(8)
    assert _same((eight[0][:, :, :4], eight[1][:, :, :4], eight[2]), four)
    again = _score(eng, mc)                                         # ... and the scoring call itself reads nothing of them
    assert np.array_equal(again[1], scores[1]) and np.array_equal(again[2], scores[2])
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ d. the facade
def test_score_alternatives_through_the_facade():
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence, alternatives_to_confmat
    from oracle import ModelConfig, make_weights, make_lines
    from oracle.decode import OracleModel
    cfg = ModelConfig(depth=2, width=64, voc_size=96)
    weights = make_weights(cfg, emb_scale=12.0)
    s2s = Sequence2Sequence()
    s2s.depth, s2s.width, s2s.batch_size = cfg.depth, cfg.width, 2
    s2s.mapping, s2s.voc_size = OracleModel(cfg, weights).mapping, cfg.voc_size
    s2s.configure()
    s2s.set_weights(weights)
    s2s.status = 2
    s2s._require_engine().set_option('deterministic', 1)
    sources, _ = make_lines(5, 12, 5, voc_size=96)
    targets, _ = make_lines(5, 10, 6, voc_size=96)
    targets[1] = ''
    targets[3] = targets[3][:4] + '\n'
    logprobs, _, predictions, ranks, _ = s2s.score_lines(sources, targets)
    K = 6
    alts, ents = s2s.score_alternatives(sources, targets, k=K)
    assert alts[1] == [] and ents[1] == []
    assert [len(a) for a in alts] == [len(t) for t in targets] == [len(e) for e in ents]
    for j in (0, 2, 3, 4):
        for u, position in enumerate(alts[j]):
            assert K - 1 <= len(position) <= K and all(ch for ch, _ in position)
            assert [lp for _, lp in position] == sorted((lp for _, lp in position), reverse=True)
            assert 0 < ents[j][u] < np.log(96)
            if len(predictions[j]) == len(alts[j]):                 # (no position's best is index 0, the entry without a character)
                assert position[0][0] == predictions[j][u]
            found = [lp for ch, lp in position if ch == targets[j][u]]
            if ranks[j][u] < K - 1:                                 # the target's tuple carries score_lines' log-probability bits
                assert found == [logprobs[j][u]], (j, u)
    # the round trip: the lists are an input of correct_lines
    live = [0, 2, 3, 4]
    conf = [alternatives_to_confmat(alts[j], floor=0.01) for j in live]
    out = s2s.correct_lines([targets[j] for j in live], conf=conf, fast=True, greedy=True, alignments=False)
    assert len(out[0]) == len(live) and all(isinstance(line, str) for line in out[0])
