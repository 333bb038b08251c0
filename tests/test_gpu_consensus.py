"""The vote over candidate lines on the device (csrc/consensus_kernels.hip: consensus_dist_kernel, consensus_risk_kernel;
csrc/consensus.hip: casv_consensus) against the restatement of tests/consensus_cases.py, which
tests/test_consensus_cases.py holds on the CPU.  Everything is compared for exact equality: int32 distances and picks, float64 risks
bit for bit.  Runs with and without CASV_POISON=1."""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

os.environ.setdefault('CASV_POISON', '1')      # read once by the library, at its first allocation

from tests import consensus_cases as cc
from tests import sample_cases as sa

ERR_ARG = -1


@pytest.fixture(scope='module')
def eng():
    """A handle without weights: the vote needs none."""
    from cor_asv_ann_amd.engine import HipEngine
    e = HipEngine(1, 32, 12)
    yield e
    e.close()


def _run(eng, sym, length, w=None, mode=0):
    return eng.consensus(sym, length, weights=w, mode=mode, want_dist=True)


def _case(name):
    return cc.cases()[cc.CASE_IDS.index(name)][1:]


# ------------------------------------------------------------------------------------------------------------------ a. the cases
@pytest.mark.parametrize('name', cc.CASE_IDS)
def test_case_against_the_restatement(eng, name):
    """Lengths 0 .. 200 against each other per alphabet, 700 x 650, 8192 x 1 and 8192 x 8190, the structured pairs, N = 1 .. 256,
    B = 1 .. 70 with padding, weights over many magnitudes in both modes, exact ties, all weights zero."""
    sym, length, w, mode = _case(name)
    got = _run(eng, sym, length, w, mode)
    want = cc.expected(name)
    assert np.array_equal(got[2], want[2]), 'distances'
    assert cc.same(got, want)
    risk, pick, _ = eng.consensus(sym, length, weights=w, mode=mode)            # without the distances: the same risks and picks
    assert cc.same((risk, pick, got[2]), want)


@pytest.mark.parametrize('how', ('other', 'random'))
@pytest.mark.parametrize('name', ('lengths_two', 'lengths_many', 'structured_65', 'weights_mode1', 'shape_N5_B70_padding'))
def test_symbols_beyond_a_length_influence_nothing(eng, name, how):
    sym, length, w, mode = _case(name)
    assert cc.same(_run(eng, cc.poisoned(sym, length, how, seed=3), length, w, mode), cc.expected(name))


def test_a_wider_L_changes_nothing(eng):
    """The same candidates in a call of L = 8192: the LDS of a wave follows the longest live candidate, not L."""
    sym, length, w, mode = _case('weights_mode1')
    wide = np.full(sym.shape[:2] + (cc.MAX_L,), 7, np.int32)
    wide[:, :, :sym.shape[2]] = sym
    assert cc.same(_run(eng, wide, length, w, mode), cc.expected('weights_mode1'))


# ------------------------------------------------------------------------------------------------------------------ b. independence
def test_sources_are_independent(eng):
    sym, length, w, mode = _case('weights_mode0')
    want = cc.expected('weights_mode0')
    B = sym.shape[0]
    perm = np.random.default_rng(0).permutation(B)
    got = _run(eng, sym[perm], length[perm], w[perm], mode)
    assert cc.same(got, tuple(x[perm] for x in want))                               # permuting the sources permutes the results
    for b in range(B):                                                              # a source alone
        assert cc.same(_run(eng, sym[b:b + 1], length[b:b + 1], w[b:b + 1], mode), tuple(x[b:b + 1] for x in want))
    # padding candidates added at the end and in front change nothing for the live ones
    N, extra = sym.shape[1], 3
    for front in (0, extra):
        s2 = np.full((B, N + extra, sym.shape[2]), 99, np.int32)
        l2 = np.full((B, N + extra), -1, np.int32)
        w2 = np.full((B, N + extra), 5.0)
        s2[:, front:front + N], l2[:, front:front + N], w2[:, front:front + N] = sym, length, w
        risk, pick, dist = _run(eng, s2, l2, w2, mode)
        keep = slice(front, front + N)
        assert cc.same((risk[:, keep], np.where(pick >= 0, pick - front, -1), dist[:, keep, keep]), want)
        rest = np.ones(N + extra, bool)
        rest[keep] = False
        assert np.isinf(risk[:, rest]).all() and (dist[:, rest] == -1).all() and (dist[:, :, rest] == -1).all()


def test_permuting_the_candidates_permutes_the_results(eng):
    sym, length, _, _ = _case('weights_mode0')
    want = cc.expected('weights_mode0')[2]
    perm = np.random.default_rng(1).permutation(sym.shape[1])
    base = _run(eng, sym, length)                                                   # unit weights, mode 0: integers in float64
    risk, pick, dist = _run(eng, sym[:, perm], length[:, perm])
    assert np.array_equal(base[2], want) and np.array_equal(dist, want[:, perm][:, :, perm])
    assert np.array_equal(risk.view(np.int64), base[0][:, perm].view(np.int64))
    assert np.array_equal(base[0], np.where(length >= 0, np.where(want >= 0, want, 0).sum(axis=2), np.inf))
    for b in range(len(pick)):                                                      # the same risk wins, at its lowest index
        assert risk[b, pick[b]] == base[0][b, base[1][b]] and pick[b] == int(np.argmin(risk[b]))


# ------------------------------------------------------------------------------------------------------------------ c. refusals
def _raw(eng, B, N, L, mode, sym, length, w, dist, risk, pick):
    from cor_asv_ann_amd import _native as nv
    return eng.lib.casv_consensus(eng.handle, B, N, L, mode, nv.ptr(sym), nv.ptr(length), nv.ptr(w), nv.ptr(dist), nv.ptr(risk), nv.ptr(pick))


def _refusals(eng):
    """Every refused argument of the header's list answers CASV_ERR_ARG and writes nothing."""
    B, N, L = 2, 3, 4
    sym, length = np.ones((B, N, L), np.int32), np.full((B, N), 2, np.int32)
    outs = lambda: (np.full((B, N, N), 77, np.int32), np.full((B, N), 77.0), np.full((B,), 77, np.int32))
    ok = dict(B=B, N=N, L=L, mode=0, sym=sym, length=length, w=None)
    bad = [dict(B=0), dict(B=-1), dict(N=0), dict(N=257), dict(L=-1), dict(L=8193), dict(mode=-1), dict(mode=2),
           dict(sym=None), dict(length=None),
           dict(length=np.array([[2, 2, -2], [2, 2, 2]], np.int32)), dict(length=np.array([[2, 2, 2], [2, 5, 2]], np.int32))]
    for v in (-1.0, -0.0 - 1e-300, np.nan, np.inf, -np.inf):
        w = np.ones((B, N))
        w[1, 2] = v
        bad.append(dict(w=w))
    for change in bad:
        dist, risk, pick = outs()
        assert _raw(eng, dist=dist, risk=risk, pick=pick, **dict(ok, **change)) == ERR_ARG, change
        assert (dist == 77).all() and (risk == 77).all() and (pick == 77).all()
    dist, risk, pick = outs()
    assert _raw(eng, dist=dist, risk=None, pick=pick, **ok) == ERR_ARG and _raw(eng, dist=dist, risk=risk, pick=None, **ok) == ERR_ARG
    assert b'' != eng.lib.casv_last_error()
    # what is allowed: no distances, L = 0 without symbols, -0.0 as a weight
    assert _raw(eng, dist=None, risk=risk, pick=pick, **ok) == 0 and (risk == 0).all() and (pick == 0).all()
    zero = np.zeros((B, N), np.int32)
    assert _raw(eng, dist=dist, risk=risk, pick=pick, **dict(ok, L=0, sym=None, length=zero, w=np.full((B, N), -0.0))) == 0
    assert (dist == 0).all() and (risk == 0).all() and (pick == 0).all()


def test_refused_arguments(eng):
    _refusals(eng)


def test_other_entry_points_are_untouched_by_the_vote():
    """A scoring and a sampling call give the same bits with a vote (served or refused) before them and between the encode and the
    decode as without."""
    from cor_asv_ann_amd.engine import HipEngine
    case = sa.BATCH_CASE
    mc = sa.build_model(case)
    model = HipEngine(case[1], case[2], case[3], **mc['flags'])
    sym, length, w, mode = _case('weights_mode1')
    try:
        assert cc.same(_run(model, sym, length, w, mode), cc.expected('weights_mode1'))      # before any weights are committed
        model.set_weights(mc['w'])
        idx = mc['idx']
        din = np.where(idx >= 0, np.roll(idx, 1, axis=1), -1).astype(np.int32)
        din[:, 0] = -1

        def others(vote):
            vote()
            model.encode(idx)
            vote()
            s = model.decode_sample(3, seed=1, temperature=0.9, top_k=5, want_align=True)
            vote()
            g = model.decode_greedy(mode=0, want_align=True)
            vote()
            t = model.score_targets(idx, None, din, idx)[:5]
            vote()
            return list(s) + list(g) + list(t)

        def vote():
            assert cc.same(_run(model, sym, length, w, mode), cc.expected('weights_mode1'))

        before = others(lambda: None)
        for between in (vote, lambda: _refusals(model)):
            after = others(between)
            for x, y in zip(before, after):
                assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()
    finally:
        model.close()


def test_the_vote_is_timed_under_its_own_class(eng):
    sym, length, _, _ = _case('ties_mode0')
    eng.profile(True)
    before = eng.profile_read('consensus')['launches']
    eng.consensus(sym, length)
    after = eng.profile_read('consensus')
    assert after['launches'] == before + 1 and after['ms'] > 0
    eng.profile(False)


# ------------------------------------------------------------------------------------------------------------------ d. end to end
FACADE_CASE = ('consensus_d1_w32_v12', 1, 32, 12, 5, 8, 6, (), False, False)       # five lines, n = 6 (tests/sample_cases.py, build_model)


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


def _points(text):
    return np.array([ord(c) for c in text], np.int32)


def _direct(cands, weights=None, mode=0):
    sym, length = cc.pack([_points(c) for c in cands])
    risk, pick = cc.risk_and_pick(cc.distance_matrix(sym, length), length, weights, mode)
    return pick, risk.tolist()


def test_consensus_lines_end_to_end():
    s2s, lines = _facade(12)
    try:
        assert len(lines) == 5 and all(line.endswith('\n') for line in lines)
        sources = lines[:2] + [''] + lines[2:]
        n, kw = 6, dict(temperature=1.3, top_k=6, seed=17)
        sampled = s2s.sample_lines(sources, n=n, **kw)
        greedy = s2s.correct_lines(sources, fast=True, greedy=True, alignments=False)[0]
        for weights in ('uniform', 'importance'):
            for normalise in (False, True):
                got = s2s.consensus_lines(sources, n=n, weights=weights, normalise=normalise, **kw)
                assert got == s2s.consensus_lines(sources, n=n, weights=weights, normalise=normalise, **kw)     # one seed: one result
                chosen, risks, cands, picks = got
                for j, line in enumerate(sources):
                    if not line:
                        assert (chosen[j], risks[j], cands[j], picks[j]) == ('', 0.0, [], None)
                        continue
                    assert cands[j] == [greedy[j]] + sampled[0][j] and len(cands[j]) == n + 1
                    w = None
                    if weights == 'importance':
                        s = [sum(float(p) - float(q) for p, q in zip(lp, lq)) for lp, lq in zip(sampled[1][j], sampled[3][j])]
                        e = [math.exp(x - max(s)) for x in s]
                        total = sum(e)
                        w = [x / total for x in e]
                        w = [sum(w) / n] + w
                    pick, risk = _direct(cands[j], w, int(normalise))
                    assert picks[j] == pick and chosen[j] == cands[j][pick] and risks[j] == risk[pick]
        assert len({c for cs in cands for c in cs}) > len(lines)                       # (the candidates are not all copies)
        # the samples alone, and the vote on its own over the same lists, in one chunk and source by source
        alone = s2s.consensus_lines(sources, n=n, include_greedy=False, **kw)
        assert alone[2] == sampled[0]
        picks, risks, dists = s2s.consensus_of(alone[2], distances=True)
        assert picks == alone[3] and [0.0 if p is None else r[p] for p, r in zip(picks, risks)] == alone[1]
        s2s.batch_size = 1
        assert s2s.consensus_of(alone[2], distances=True) == (picks, risks, dists)
        for j, cs in enumerate(alone[2]):
            if cs:
                assert (picks[j], risks[j]) == _direct(cs)
                assert dists[j] == cc.distance_matrix(*cc.pack([_points(c) for c in cs])).tolist()
    finally:
        s2s.engine.close()


def test_consensus_of_votes_on_lines_from_outside_the_model():
    """An unconfigured facade, characters no model here knows, non-BMP among them."""
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence
    s2s = Sequence2Sequence()
    cands = [['Fraktur \U0001D509\n', 'Fraktur \U0001D50A\n', 'Fraktur \U0001D509\n'], [], ['ſ', '', 's', 'ſ̈']]
    try:
        picks, risks, dists = s2s.consensus_of(cands, weights=[None, None, [1.0, 0.5, 2.0, 0.25]], normalise=True, distances=True)
        assert picks[1] is None and risks[1] == [] and dists[1] == []
        assert dists[0] == [[0, 1, 0], [1, 0, 1], [0, 1, 0]] and dists[2] == [[0, 1, 1, 1], [1, 0, 1, 2], [1, 1, 0, 2], [1, 2, 2, 0]]
        assert (picks[0], risks[0]) == _direct(cands[0], None, 1) and (picks[2], risks[2]) == _direct(cands[2], [1.0, 0.5, 2.0, 0.25], 1)
    finally:
        s2s._vote_engine.close()
