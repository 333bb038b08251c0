"""The confusion network voted from candidate lines on the device (csrc/consensus_kernels.hip: consensus_align_kernel,
consensus_layout_kernel, consensus_vote_kernel; csrc/consensus_align.hip: casv_consensus_align, casv_consensus_vote; DESIGN.md
section 4.10) against the restatement of tests/align_cases.py, which tests/test_align_cases.py holds on the CPU.  Everything is
compared for exact equality: int32 where, ncol, src and best, float64 masses bit for bit.  Runs with and without CASV_POISON=1."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

os.environ.setdefault('CASV_POISON', '1')      # read once by the library, at its first allocation

from tests import align_cases as ac
from tests import consensus_cases as cc
from tests import sample_cases as sa

ERR_ARG, ERR_STATE = -1, -2


@pytest.fixture(scope='module')
def eng():
    """A handle without weights: the pair needs none."""
    from cor_asv_ann_amd.engine import HipEngine
    e = HipEngine(1, 32, 12)
    yield e
    e.close()


def _run(eng, sym, length, pivot, w=None, C=None):
    """(where, ncol, src, mass, best) of an align and one vote at C columns (None: the largest ncol, at least 1)."""
    where, ncol = eng.consensus_align(sym, length, pivot)
    return (where, ncol) + eng.consensus_vote(max(1, int(ncol.max())) if C is None else C, weights=w)


def _stat(eng, key):
    from ctypes import byref, c_int64
    value = c_int64()
    assert eng.lib.casv_get_stat(eng.handle, key.encode(), byref(value)) == 0
    return value.value


# ------------------------------------------------------------------------------------------------------------------ a. the cases
@pytest.mark.parametrize('name', ac.CASE_IDS)
def test_case_against_the_restatement(eng, name):
    """Lengths 0 .. 200 against each other per alphabet with the edges of a direction word, 2048 x 2047, 2048 x 1 and 1 x 2048,
    the structured pairs, N = 1 .. 256, B = 1 .. 70 with padding and skipped sources, 66 000 sources, weights over many
    magnitudes, exact ties, all weights zero, the order of the sum."""
    sym, length, pivot, w = ac.case(name)
    got = _run(eng, sym, length, pivot, w)
    want = ac.expected(name)
    assert np.array_equal(got[0], want[0]), 'where'
    assert np.array_equal(got[1], want[1]), 'ncol'
    assert np.array_equal(got[2], want[2]), 'src'
    assert ac.same(got, want)


@pytest.mark.parametrize('how', ('other', 'random'))
@pytest.mark.parametrize('name', ('lengths_two', 'lengths_many', 'structured_65', 'weights', 'shape_N5_B70_padding'))
def test_symbols_beyond_a_length_influence_nothing(eng, name, how):
    sym, length, pivot, w = ac.case(name)
    assert ac.same(_run(eng, cc.poisoned(sym, length, how, seed=3), length, pivot, w), ac.expected(name))


def test_a_wider_L_changes_nothing(eng):
    """The same candidates in a call of L = 2048: LDS and direction words follow the longest live candidate, not L."""
    sym, length, pivot, w = ac.case('weights')
    wide = np.full(sym.shape[:2] + (ac.MAX_L,), 7, np.int32)
    wide[:, :, :sym.shape[2]] = sym
    got = _run(eng, wide, length, pivot, w)
    want = ac.expected('weights')
    assert (got[0][:, :, sym.shape[2]:] == ac.NONE).all()
    assert ac.same((got[0][:, :, :sym.shape[2]],) + got[1:], want)


def test_more_columns_than_needed(eng):
    """C exact and C larger: the columns beyond a source's ncol hold src -2, mass -1.0, best -1."""
    sym, length, pivot, w = ac.case('weights')
    want = ac.expected('weights')
    C = int(want[1].max())
    ref = ac.Reference()
    ref.align(sym, length, pivot)
    for more in (0, 1, 37):
        got = _run(eng, sym, length, pivot, w, C=C + more)
        assert ac.same(got, want[:2] + ref.vote(C + more, w))
        assert (got[2][:, C:] == -2).all() and (got[3][:, C:] == -1.0).all() and (got[4][:, C:] == -1).all()


# ------------------------------------------------------------------------------------------------------------------ b. independence
def test_sources_are_independent(eng):
    sym, length, pivot, w = ac.case('weights')
    want = ac.expected('weights')
    B = sym.shape[0]
    C = want[2].shape[1]
    perm = np.random.default_rng(0).permutation(B)
    got = _run(eng, sym[perm], length[perm], pivot[perm], w[perm])
    assert ac.same(got, tuple(x[perm] for x in want))                               # permuting the sources permutes the results
    for b in range(B):                                                              # a source alone
        got = _run(eng, sym[b:b + 1], length[b:b + 1], pivot[b:b + 1], w[b:b + 1], C=C)
        assert ac.same(got, tuple(x[b:b + 1] for x in want))


def test_permuting_the_candidates_permutes_the_results(eng):
    """The pivot index follows its candidate: the same alignments, columns and classes; a class is then represented by the member
    that comes first in the new order, with the members' weights added in the new order."""
    sym, length, pivot, w = ac.case('weights')
    want = ac.expected('weights')
    N = sym.shape[1]
    perm = np.random.default_rng(1).permutation(N)
    inverse = np.argsort(perm)
    moved = np.where(pivot >= 0, inverse[np.maximum(pivot, 0)], -1).astype(np.int32)
    got = _run(eng, sym[:, perm], length[:, perm], moved, w[:, perm])
    assert ac.same(got, ac.reference(sym[:, perm], length[:, perm], moved, w[:, perm]))
    assert np.array_equal(got[0], want[0][:, perm]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2][:, :, perm])
    # unit weights: the masses are small integers, exact in any order -- the same classes with the same masses
    unit, base = _run(eng, sym[:, perm], length[:, perm], moved), _run(eng, sym, length, pivot)
    assert np.array_equal(np.sort(unit[3], axis=2), np.sort(base[3], axis=2))
    assert np.array_equal(np.take_along_axis(unit[3], np.maximum(unit[4], 0)[:, :, None], 2), np.take_along_axis(base[3], np.maximum(base[4], 0)[:, :, None], 2))


@pytest.mark.parametrize('name,budget,rounds', [('weights', 1, 6), ('shape_N5_B70_padding', 1, 70), ('lengths_two', 4 * 13 * 200 * 7 * 8, 4)])
def test_rounds_under_a_small_budget_change_nothing(eng, name, budget, rounds):
    """The direction words of a call that do not fit the budget are filled and walked in rounds of sources (at least one source a
    round): the same bits as in one round."""
    sym, length, pivot, w = ac.case(name)
    assert ac.same(_run(eng, sym, length, pivot, w), ac.expected(name)) and _stat(eng, 'align_rounds') == 1
    eng.debug_set_align_budget(budget)
    try:
        got = _run(eng, sym, length, pivot, w)
        assert _stat(eng, 'align_rounds') == rounds >= 3
    finally:
        eng.debug_set_align_budget(0)
    assert ac.same(got, ac.expected(name))


def test_votes_again_with_other_weights_and_a_distance_vote_between(eng):
    """One align, then votes with these weights, none, others and the first again, with a casv_consensus call in between."""
    sym, length, pivot, w = ac.case('weights')
    want = ac.expected('weights')
    ref = ac.Reference()
    ref.align(sym, length, pivot)
    C = want[2].shape[1]
    where, ncol = eng.consensus_align(sym, length, pivot)
    assert ac.same((where, ncol), want[:2])
    other = np.random.default_rng(5).random(w.shape)
    other[:, 3] = 0.0
    vsym, vlength, vw, mode = cc.cases()[cc.CASE_IDS.index('weights_mode1')][1:]
    for weights in (w, None, other, w):
        assert ac.same(eng.consensus_vote(C, weights=weights), ref.vote(C, weights))
        assert cc.same(eng.consensus(vsym, vlength, weights=vw, mode=mode, want_dist=True), cc.expected('weights_mode1'))


# ------------------------------------------------------------------------------------------------------------------ c. refusals
def _raw_align(eng, B, N, L, sym, length, pivot, where, ncol):
    from cor_asv_ann_amd import _native as nv
    return eng.lib.casv_consensus_align(eng.handle, B, N, L, nv.ptr(sym), nv.ptr(length), nv.ptr(pivot), nv.ptr(where), nv.ptr(ncol))


def _raw_vote(eng, C, w, src, mass, best):
    from cor_asv_ann_amd import _native as nv
    return eng.lib.casv_consensus_vote(eng.handle, C, nv.ptr(w), nv.ptr(src), nv.ptr(mass), nv.ptr(best))


def _refusals(eng):
    """After a served align: every refused argument of the header's list answers CASV_ERR_ARG and writes nothing, and a vote
    afterwards still reads the served align."""
    sym, length, pivot, w = ac.case('ties_weighted')
    want = ac.expected('ties_weighted')
    kept_B, kept_N = length.shape
    kept_C = want[2].shape[1]
    assert ac.same(_run(eng, sym, length, pivot, w), want)
    B, N, L = 2, 3, 4
    bsym, blength, bpivot = np.ones((B, N, L), np.int32), np.array([[2, 2, -1], [2, 0, 4]], np.int32), np.array([1, -1], np.int32)
    outs = lambda: (np.full((B, N, L), 77, np.int32), np.full((B,), 77, np.int32))
    ok = dict(B=B, N=N, L=L, sym=bsym, length=blength, pivot=bpivot)
    bad = [dict(B=0), dict(B=-1), dict(N=0), dict(N=257), dict(L=-1), dict(L=2049), dict(sym=None), dict(length=None), dict(pivot=None),
           dict(length=np.array([[2, 2, -2], [2, 2, 2]], np.int32)), dict(length=np.array([[2, 2, 2], [2, 5, 2]], np.int32)),
           dict(pivot=np.array([3, 0], np.int32)), dict(pivot=np.array([0, -2], np.int32)), dict(pivot=np.array([2, 0], np.int32))]
    for change in bad:
        where, ncol = outs()
        assert _raw_align(eng, where=where, ncol=ncol, **dict(ok, **change)) == ERR_ARG, change
        assert (where == 77).all() and (ncol == 77).all()
    where, ncol = outs()
    assert _raw_align(eng, where=None, ncol=ncol, **ok) == ERR_ARG and _raw_align(eng, where=where, ncol=None, **ok) == ERR_ARG
    assert (where == 77).all() and (ncol == 77).all() and b'' != eng.lib.casv_last_error()
    vouts = lambda: (np.full((kept_B, kept_C, kept_N), 77, np.int32), np.full((kept_B, kept_C, kept_N), 77.0), np.full((kept_B, kept_C), 77, np.int32))
    src, mass, best = vouts()
    for C in (0, -1, kept_C - 1):
        assert _raw_vote(eng, C, None, src, mass, best) == ERR_ARG
    for v in (-1.0, -0.0 - 1e-300, np.nan, np.inf, -np.inf):
        bw = np.ones((kept_B, kept_N))
        bw[1, 2] = v
        assert _raw_vote(eng, kept_C, bw, src, mass, best) == ERR_ARG
    assert _raw_vote(eng, kept_C, None, None, mass, best) == ERR_ARG and _raw_vote(eng, kept_C, None, src, None, best) == ERR_ARG
    assert _raw_vote(eng, kept_C, None, src, mass, None) == ERR_ARG
    assert (src == 77).all() and (mass == 77).all() and (best == 77).all()
    # the served align is still there, whole
    assert _raw_vote(eng, kept_C, w, src, mass, best) == 0 and ac.same((src, mass, best), want[2:])
    # what is allowed: L = 0 without symbols or where, -0.0 as a weight
    ncol = np.full((B,), 77, np.int32)
    assert _raw_align(eng, B, N, 0, None, np.array([[0, 0, -1], [-1, 0, 0]], np.int32), np.array([0, 2], np.int32), None, ncol) == 0
    assert ncol.tolist() == [0, 0]
    src, mass, best = np.full((B, 1, N), 77, np.int32), np.full((B, 1, N), 77.0), np.full((B, 1), 77, np.int32)
    assert _raw_vote(eng, 1, np.full((B, N), -0.0), src, mass, best) == 0
    assert (src == -2).all() and (mass == -1.0).all() and (best == -1).all()


def test_refused_arguments(eng):
    _refusals(eng)


def test_a_vote_without_an_align_is_a_state_error():
    from cor_asv_ann_amd.engine import HipEngine
    from cor_asv_ann_amd import _native as nv
    fresh = HipEngine(1, 32, 12)
    try:
        src, mass, best = np.full((1, 1, 1), 77, np.int32), np.full((1, 1, 1), 77.0), np.full((1, 1), 77, np.int32)
        assert _raw_vote(fresh, 1, None, src, mass, best) == ERR_STATE
        assert (src == 77).all() and (mass == 77).all() and (best == 77).all()
        with pytest.raises(nv.NativeError):
            fresh.consensus_vote(1)
        # a refused align leaves it at that
        ncol = np.full((1,), 77, np.int32)
        assert _raw_align(fresh, 1, 1, 0, None, np.array([[0]], np.int32), np.array([5], np.int32), None, ncol) == ERR_ARG
        assert _raw_vote(fresh, 1, None, src, mass, best) == ERR_STATE
    finally:
        fresh.close()


def test_other_entry_points_are_untouched_by_the_pair():
    """The distance vote, a sampling call, a greedy decode and a scoring call give the same bits with align / vote calls (served or
    refused) before, between and behind them as without; the pair runs before any weights exist."""
    from cor_asv_ann_amd.engine import HipEngine
    case = sa.BATCH_CASE
    mc = sa.build_model(case)
    model = HipEngine(case[1], case[2], case[3], **mc['flags'])
    sym, length, pivot, w = ac.case('weights')
    vsym, vlength, vw, vmode = cc.cases()[cc.CASE_IDS.index('weights_mode1')][1:]
    try:
        assert ac.same(_run(model, sym, length, pivot, w), ac.expected('weights'))          # before any weights are committed
        model.set_weights(mc['w'])
        idx = mc['idx']
        din = np.where(idx >= 0, np.roll(idx, 1, axis=1), -1).astype(np.int32)
        din[:, 0] = -1

        def others(pair):
            pair()
            v = model.consensus(vsym, vlength, weights=vw, mode=vmode, want_dist=True)
            pair()
            model.encode(idx)
            pair()
            s = model.decode_sample(3, seed=1, temperature=0.9, top_k=5, want_align=True)
            pair()
            g = model.decode_greedy(mode=0, want_align=True)
            pair()
            t = model.score_targets(idx, None, din, idx)[:5]
            pair()
            return list(v) + list(s) + list(g) + list(t)

        def pair():
            assert ac.same(_run(model, sym, length, pivot, w), ac.expected('weights'))

        before = others(lambda: None)
        assert cc.same(before[:3], cc.expected('weights_mode1'))
        for between in (pair, lambda: _refusals(model)):
            after = others(between)
            for x, y in zip(before, after):
                assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()
        # an align, the other entry points, then the vote: it still reads that align
        where, ncol = model.consensus_align(sym, length, pivot)
        others(lambda: None)
        want = ac.expected('weights')
        assert ac.same((where, ncol) + model.consensus_vote(want[2].shape[1], weights=w), want)
    finally:
        model.close()


def test_the_pair_is_timed_under_the_vote_s_class(eng):
    sym, length, pivot, _ = ac.case('ties')
    eng.profile(True)
    before = eng.profile_read('consensus')['launches']
    _, ncol = eng.consensus_align(sym, length, pivot)
    middle = eng.profile_read('consensus')
    assert middle['launches'] == before + 1 and middle['ms'] > 0                   # one record per call
    eng.consensus_vote(int(ncol.max()))
    after = eng.profile_read('consensus')
    assert after['launches'] == before + 2 and after['ms'] > middle['ms']
    eng.profile(False)


# ------------------------------------------------------------------------------------------------------------------ d. end to end
FACADE_CASE = ('confusion_d1_w32_v12', 1, 32, 12, 5, 8, 6, (), False, False)       # five lines, n = 6 (tests/sample_cases.py, build_model)


def _facade(batch_size):
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence
    from oracle.decode import OracleModel
    mc = sa.build_model(FACADE_CASE)
    s2s = Sequence2Sequence()
    s2s.depth, s2s.width, s2s.batch_size = FACADE_CASE[1], FACADE_CASE[2], batch_size
    s2s.mapping, s2s.voc_size = OracleModel(mc['cfg'], mc['w']).mapping, FACADE_CASE[3]
    s2s.configure()
    s2s.set_weights(mc['w'])
    s2s.status = 2
    i_c = s2s.mapping[1]
    return s2s, [''.join(i_c[int(i)] for i in row if i >= 0) for row in mc['idx']]


def _helper(candidates, weights=None, pivots=None, normalise=False, floor=0.0):
    """confusion_of on the stub engine: the same facade code over the restatement."""
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence
    stub = Sequence2Sequence()
    stub.batch_size, stub.engine = 7, ac.StubEngine()
    return stub.confusion_of(candidates, weights=weights, pivots=pivots, normalise=normalise, floor=floor)


def test_confusion_of_and_correct_candidates_end_to_end():
    s2s, lines = _facade(12)
    try:
        assert len(lines) == 5 and all(line.endswith('\n') for line in lines)
        sources = lines[:2] + [''] + lines[2:]
        candidates = s2s.sample_lines(sources, n=6, temperature=1.3, top_k=6, seed=17)[0]
        assert candidates[2] == [] and len({c for cs in candidates for c in cs}) > len(lines)      # (not all copies)
        weights = [None if not cs else [1.0 + 0.25 * k for k in range(len(cs))] for cs in candidates]
        for kw in (dict(), dict(weights=weights, normalise=True, floor=0.2), dict(pivots=[None if not cs else len(cs) - 1 for cs in candidates])):
            got = s2s.confusion_of(candidates, **kw)
            assert got == s2s.confusion_of(candidates, **kw) == _helper(candidates, **kw)
            voted, confmats, pivots, columns = got
            assert (voted[2], confmats[2], pivots[2], columns[2]) == ('', [], None, [])
            assert all(''.join(chunk[0][0] for chunk in confmat) == line for confmat, line in zip(confmats, voted))
            s2s.batch_size = 1                                                                       # source by source
            assert s2s.confusion_of(candidates, **kw) == got
            s2s.batch_size = 12
            # the model's correction of the voted networks, against the same call made by hand
            corrected = s2s.correct_candidates(candidates, alignments=False, **kw)
            live = [j for j in range(len(sources)) if confmats[j]]
            by_hand = s2s.correct_lines([voted[j] for j in live], conf=[confmats[j] for j in live], fast=True, greedy=True, alignments=False)
            assert [corrected[0][j] for j in live] == by_hand[0] and [corrected[1][j] for j in live] == by_hand[1]
            assert [corrected[2][j] for j in live] == by_hand[2] and any(by_hand[0])
            assert (corrected[0][2], corrected[1][2], corrected[2][2], corrected[3][2]) == ('', [], 0.0, [])
        eng = s2s.engine
        s2s.batch_size = 100                                                                         # (one chunk)
        eng.profile(True)
        s2s.confusion_of(candidates, pivots=[None if not cs else 0 for cs in candidates])
        assert eng.profile_read('consensus')['launches'] == 2                                      # one align, one vote; nothing else ran
        eng.profile(False)
    finally:
        s2s.engine.close()


def test_confusion_of_votes_on_lines_from_outside_the_model():
    """An unconfigured facade, characters no model here knows, non-BMP among them: three readings of a line, one pivot."""
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence
    s2s = Sequence2Sequence()
    cands = [['Fraktur \U0001D509\n', 'Fraktnr \U0001D50A\n', 'Fraktur\U0001D509\n'], [], ['ſ', '', 's', 'ſ̈']]
    try:
        got = s2s.confusion_of(cands, weights=[None, None, [1.0, 0.5, 2.0, 0.25]])
        assert got == _helper(cands, weights=[None, None, [1.0, 0.5, 2.0, 0.25]])
        assert got[0] == ['Fraktur \U0001D509\n', '', 's'] and got[2] == [0, None, 2]
        assert got[1][0][5] == [('u', 2 / 3), ('n', 1 / 3)] and got[1][0][7] == [(' ', 2 / 3), ('', 1 / 3)]
        # the pivot 's': the last candidate's diaeresis stands against it and its long s in front -- the diagonal goes first
        assert got[1][2] == [[('', 3.5 / 3.75), ('ſ', 0.25 / 3.75)], [('s', 2.0 / 3.75), ('ſ', 1.0 / 3.75), ('', 0.5 / 3.75), ('̈', 0.25 / 3.75)]]
    finally:
        s2s._vote_engine.close()
