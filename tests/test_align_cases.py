"""tests/align_cases.py held on the CPU: the restated alignment against answers made by hand and against the project's own edit
distance, the structure of `where` and of the columns, the rules of the vote, the case list the device runs, and the facade
(confusion_of, correct_candidates) on a stub engine that answers from the restatement.  The device's side:
tests/test_gpu_confusion.py."""
import math
import os

import numpy as np
import pytest

from tests import align_cases as ac
from tests import consensus_cases as cc


def _points(text):
    return np.array([ord(c) for c in text], np.int32)


def _source(texts, pivot, weights=None):
    """One source from strings (None: padding): (where (N,L), ncol, src (ncol,N), mass (ncol,N), best (ncol))."""
    sym, length = cc.pack([None if t is None else _points(t) for t in texts])
    where, ncol, src = ac.align_source(sym, length, pivot)
    return (where, ncol, src) + ac.vote_source(sym, length, src, weights)


# ------------------------------------------------------------------------------------------------------------------ 1. the alignment
def test_answers_made_by_hand():
    where, cost = ac.walk(_points('kitten'), _points('sitting'))
    assert where.tolist() == [0, 1, 2, 3, 4, 5, -7] and cost == 3               # k/s, e/i, and g behind the last symbol: slot 6
    where, cost = ac.walk(_points('sitting'), _points('kitten'))
    assert where.tolist() == [0, 1, 2, 3, 4, 5] and cost == 3                   # the pivot's g, its last symbol, stands against a gap
    # the pivot 'ab' against 'b', 'a', '' and 'xaby'
    where, ncol, src, mass, best = _source(['ab', 'b', 'a', '', 'xaby'], 0)
    assert [where[c, :n].tolist() for c, n in enumerate([2, 1, 1, 0, 4])] == [[0, 1], [1], [0], [], [-1, 0, 1, -3]]
    assert (where[1, 1:] == ac.NONE).all() and (where[3] == ac.NONE).all()
    assert ncol == 4                                                            # x in slot 0, a, b, y in slot 2
    assert src.tolist() == [[-1, -1, -1, -1, 0], [0, -1, 0, -1, 1], [1, 0, -1, -1, 2], [-1, -1, -1, -1, 3]]
    assert mass.tolist() == [[4, -1, -1, -1, 1], [3, 2, -1, -1, -1], [3, -1, 2, -1, -1], [4, -1, -1, -1, 1]]
    assert best.tolist() == [0, 0, 0, 0]
    # one symbol only, where every move ties: the diagonal goes first, so the shorter line stands against the END of the longer
    assert ac.walk(_points('aaa'), _points('aa'))[0].tolist() == [1, 2]
    assert ac.walk(_points('aa'), _points('aaa'))[0].tolist() == [-1, 0, 1]
    assert ac.walk(_points('aaaa'), _points('a'))[0].tolist() == [3]
    # an empty pivot: everything is inserted in slot 0; an empty candidate: nothing to say
    assert ac.walk(_points(''), _points('abc'))[0].tolist() == [-1, -1, -1] and ac.walk(_points('abc'), _points(''))[0].tolist() == []
    where, ncol, src, mass, best = _source(['', 'abc', 'xb', None], 0)
    assert ncol == 3 and src.tolist() == [[-1, 0, 0, -2], [-1, 1, 1, -2], [-1, 2, -1, -2]]
    assert mass.tolist() == [[1, 1, 1, -1], [1, 2, -1, -1], [2, 1, -1, -1]] and best.tolist() == [0, 1, 0]
    # symbols are compared for equality only: any int32 is one
    assert ac.walk(np.array([cc.I32_MIN, 0, cc.I32_MAX]), np.array([cc.I32_MIN, cc.I32_MAX]))[0].tolist() == [0, 2]


def test_path_cost_against_the_project_s_own_distance():
    from cor_asv_ann_amd.metrics import Alignment
    rng = np.random.default_rng(1)
    for trial in range(150):
        alphabet = [[3], [0, 1], list(range(30))][trial % 3]
        a = cc._draw(rng, alphabet, int(rng.integers(0, 70)))
        b = cc._mutate(rng, a, alphabet, int(rng.integers(0, 12))) if trial % 2 else cc._draw(rng, alphabet, int(rng.integers(0, 70)))
        where, cost = ac.walk(a, b)
        assert cost == Alignment.get_levenshtein_distance(a.tolist(), b.tolist())[0] == cc.levenshtein(a, b)
        # the cost read off `where` alone: substitutions, pivot symbols without a partner, insertions
        hit = where >= 0
        assert cost == int((a[where[hit]] != b[hit]).sum()) + (len(a) - int(hit.sum())) + int((~hit).sum())


def test_structure():
    rng = np.random.default_rng(2)
    for trial in range(60):
        alphabet = [[3], [0, 1], list(range(30))][trial % 3]
        N = int(rng.integers(1, 7))
        strings = [cc._draw(rng, alphabet, int(rng.choice([0, 1, 2, 5, 17, 33, 64, 65]))) if rng.random() > 0.15 else None for _ in range(N)]
        if all(s is None for s in strings):
            strings[0] = cc._draw(rng, alphabet, 3)
        sym, length = cc.pack(strings, L=70)
        pivot = int(rng.choice(np.nonzero(length >= 0)[0]))
        where, ncol, src = ac.align_source(sym, length, pivot)
        lp = int(length[pivot])
        assert where[pivot, :lp].tolist() == list(range(lp))                    # the pivot against itself: the identity
        most = np.zeros(lp + 1, int)
        for c in range(N):
            n = int(length[c])
            if n < 0:
                assert (where[c] == ac.NONE).all() and (src[:, c] == -2).all()
                continue
            w = where[c, :n].astype(int)
            assert (where[c, n:] == ac.NONE).all()
            slot = np.where(w >= 0, w, -1 - w)
            assert (np.diff(slot) >= 0).all() and (np.diff(w[w >= 0]) > 0).all() and slot.max(initial=0) <= lp    # monotone
            assert ((w >= 0)[1:] | (slot[1:] > slot[:-1]) | (w[:-1] < 0)).all()    # in a slot's range the insertions come first
            most = np.maximum(most, np.bincount(-1 - w[w < 0], minlength=lp + 1))
            put = src[:, c][src[:, c] >= 0]
            assert put.tolist() == list(range(n)) and (src[:, c] >= -1).all()    # every symbol in exactly one column, in order
        assert ncol == lp + most.sum() == len(src)
        assert (src[:, pivot] >= 0).sum() == lp and ((src >= 0).any(axis=1)).all()     # no column without a symbol


# ------------------------------------------------------------------------------------------------------------------ 2. the vote
def test_vote_rules():
    # the order of the float64 sum is the candidates' order
    _, _, _, mass, best = _source(['a', 'a', 'a'], 0, [1e16, 1.0, 1.0])
    assert mass.tolist() == [[1e16, -1.0, -1.0]]
    _, _, _, mass, best = _source(['a', 'a', 'a'], 2, [1.0, 1.0, 1e16])
    assert mass.tolist() == [[1e16 + 2.0, -1.0, -1.0]] and 1e16 + 2.0 != 1e16
    # ties go to the lower index, whichever class that is; a padding candidate's weight is not read
    _, _, _, mass, best = _source(['a', 'b', 'b', 'a'], 0)
    assert mass.tolist() == [[2, 2, -1, -1]] and best.tolist() == [0]
    _, _, _, mass, best = _source(['b', None, 'a', 'a', 'b', ''], 4, [1.0, 50.0, 0.5, 1.5, 1.0, 2.0])
    assert mass.tolist() == [[2, -1, 2, -1, -1, 2]] and best.tolist() == [0]
    _, _, _, mass, best = _source(['b', 'a', '', ''], 1, [1.0, 1.0, 1.0, 1.5])
    assert mass.tolist() == [[1, 1, 2.5, -1]] and best.tolist() == [2]             # the gap wins: the voted line is empty
    _, _, _, mass, best = _source(['a', 'b'], 0, [0.0, 0.0])
    assert mass.tolist() == [[0, 0]] and best.tolist() == [0] and math.copysign(1.0, mass[0, 0]) == 1.0
    # beyond ncol: src -2, mass -1.0, best -1; a skipped source has no columns
    sym, length = cc.pack([_points('ab'), _points('b')])
    got = ac.reference(np.stack([sym, sym]), np.stack([length, length]), np.array([0, -1], np.int32), C=3)
    assert got[1].tolist() == [2, 0] and (got[0][1] == ac.NONE).all()
    assert got[2][0].tolist() == [[0, -1], [1, 0], [-2, -2]] and (got[2][1] == -2).all()
    assert got[3][0].tolist() == [[1, 1], [2, -1], [-1, -1]] and (got[3][1] == -1).all()
    assert got[4].tolist() == [[0, 0, -1], [-1, -1, -1]]


def test_the_case_list_is_the_issue_s():
    cases = {c[0]: c for c in ac.cases()}
    assert len(cases) == len(ac.cases())
    for name in ('one', 'two', 'many'):
        _, sym, length, pivot, _ = cases['lengths_' + name]
        assert length[0].tolist() == [0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200] and (length == length[0]).all()
        assert pivot.tolist() == list(range(13))                                    # every length as the pivot of all the others
        assert len(np.unique(sym)) <= max(len(cc.ALPHABETS[name]), 2)
    many = set(cases['lengths_many'][1].ravel().tolist())
    assert {0, 0x10FFFF, cc.I32_MAX}.issubset(many) and min(many) < 0
    _, sym, length, pivot, _ = cases['pairs_2048']
    assert [(int(l[p]), int(l[1 - p])) for l, p in zip(length, pivot)] == [(2048, 2047), (2048, 1), (1, 2048)] and len(np.unique(sym)) == 2
    assert sorted(c[1].shape[1] for c in cases.values() if c[0].startswith('shape_N') and 'padding' not in c[0]) == ac.SHAPE_N
    assert cases['shape_N256_B17'][1].shape[0] == 17
    assert sorted(c[1].shape[0] for c in cases.values() if c[0].endswith('_padding')) == [1, 3, 70]
    length = np.concatenate([c[2] for c in cases.values() if c[0].endswith('_padding')])
    pivot = np.concatenate([c[3] for c in cases.values() if c[0].endswith('_padding')])
    assert (length[:, 0] < 0).any() and (length[:, 2] < 0).any() and (length[:, 4] < 0).any() and (length < 0).all(axis=1).any()
    assert (pivot[(length >= 0).any(axis=1)] == -1).any()                           # a source with candidates that is skipped
    lots = cases['sources_%d' % ac.MANY_SOURCES]
    assert lots[1].shape == (ac.MANY_SOURCES, 2, 3) and ac.MANY_SOURCES > 65535 and set(lots[3].tolist()) == {-1, 0, 1}
    for name, sym, length, pivot, w in ac.cases():
        assert sym.dtype == np.int32 and length.dtype == np.int32 and pivot.dtype == np.int32
        assert sym.shape[:2] == length.shape and pivot.shape == sym.shape[:1]
        assert 1 <= sym.shape[1] <= ac.MAX_N and sym.shape[2] <= ac.MAX_L and length.min() >= -1 and length.max() <= sym.shape[2]
        assert all(p == -1 or (0 <= p < sym.shape[1] and length[b, p] >= 0) for b, p in enumerate(pivot))
        assert w is None or (w.shape == length.shape and w.dtype == np.float64 and np.isfinite(w).all() and (w >= 0).all())
    w = cases['weights'][4]
    assert (w == 0).any() and np.log10(w[w > 0].max()) - np.log10(w[w > 0].min()) > 100
    # the structured sources: the pivot is equal to, a prefix of, an extension of and the reverse of a candidate
    for n in (64, 65, 130):
        where, ncol = ac.expected('structured_%d' % n)[:2]
        assert where[0, 1, :n].tolist() == list(range(n)) and ncol[0] >= n + 9 and ncol[1] >= n + 9
        assert where[0, 6, n:n + 9].tolist() == [-1 - n] * 9 and where[1, 0, :n].tolist() == list(range(n))
    _, _, _, mass, best = ac.expected('ties')
    differ = [3, 17, 29]
    assert (mass[0, differ, :2] == 2).all() and (mass[1, differ, :2] == 2).all() and (best[:2] == 0).all() and (best[2] == 1).all()
    assert (ac.expected('all_weights_zero')[3].max(axis=2) == 0).all() and (ac.expected('all_weights_zero')[4] == 0).all()
    mass = ac.expected('sum_order')[3]
    assert (mass[0, :, 0] == 1e16).all() and (mass[1, :, 0] == 1e16 + 2).all()
    where, ncol, src, mass, best = ac.expected('shape_N5_B70_padding')
    skipped = cases['shape_N5_B70_padding'][3] < 0
    assert skipped.any() and (ncol[skipped] == 0).all() and (where[skipped] == ac.NONE).all() and (best[skipped] == -1).all()


def test_poison_leaves_the_results_alone():
    sym, length, pivot, w = ac.case('weights')
    for how in ('other', 'random'):
        p = cc.poisoned(sym, length, how)
        assert not np.array_equal(p, sym)
        assert ac.same(ac.reference(p, length, pivot, w)[:2] + ac.reference(p, length, pivot, w)[3:], ac.expected('weights')[:2] + ac.expected('weights')[3:])


# ------------------------------------------------------------------------------------------------------------------ 3. the facade
def _stub_facade(batch_size, status=0):
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence
    s2s = Sequence2Sequence()
    s2s.batch_size = batch_size
    s2s.engine = ac.StubEngine()
    s2s.status = status
    return s2s


# (outside the Basic Multilingual Plane, and characters no mapping of the tests has)
CANDIDATES = [['Fraktur \U0001D509\n', 'Fraktur \U0001D50A\n', 'Fraktur \U0001D509\n'],
              [],
              ['long s: ſ\n', '', 'long s: s\n', 'long ſ: s\n', 'lonɡ s: ſ\n'],
              ['a\n'],
              ['\U0010FFFF', '\U0010FFFF\U0010FFFF'],
              ['x\n', 'y\n', 'x\n', 'y\n'],
              ['', '']]


def _direct(cands, pivot, weights=None, floor=0.0):
    """(line, confmat, columns) of one source from the restatement, assembled with plain loops."""
    sym, length = cc.pack([_points(c) for c in cands])
    _, ncol, src = ac.align_source(sym, length, pivot)
    mass, best = ac.vote_source(sym, length, src, weights)
    total = 0.0
    for k in range(len(cands)):
        total = total + (1.0 if weights is None else float(weights[k]))
    line, confmat, columns = '', [], []
    for col in range(ncol):
        char = lambda c: '' if src[col, c] < 0 else cands[c][src[col, c]]
        reps = [c for c in range(len(cands)) if mass[col, c] >= 0]
        order = sorted(reps, key=lambda c: (-mass[col, c], c))
        assert order[0] == best[col]
        columns.append([(char(c), float(mass[col, c]), [k for k in range(len(cands)) if char(k) == char(c)]) for c in order])
        alts = [(char(c), float(mass[col, c]) / total) for c in order]
        confmat.append(alts[:1] + [a for a in alts[1:] if a[1] >= floor])
        line += char(order[0])
    return line, confmat, columns


def test_confusion_of_chunks_pads_and_converts():
    s2s = _stub_facade(12)                                    # works on an empty model: status 0, no vocabulary
    lines, confmats, pivots, columns = s2s.confusion_of(CANDIDATES)
    calls = s2s.engine.calls
    # first consensus_of's picks (three chunks), then per chunk an align and a vote
    assert [c[0] if isinstance(c[0], str) else 'consensus' for c in calls] == ['consensus'] * 3 + ['align', 'vote'] * 3
    assert pivots == [0, None, 0, 0, 0, 0, 0] == s2s.consensus_of(CANDIDATES)[0]
    aligns = [c for c in calls if isinstance(c[0], str) and c[0] == 'align']
    assert [c[1].shape for c in aligns] == [(2, 5, 10), (3, 4, 2), (1, 2, 0)]            # (the last: nothing but empty candidates, L = 0)
    assert aligns[0][2].tolist() == [[10, 10, 10, -1, -1], [10, 0, 10, 10, 10]]                 # padding candidates: -1
    assert aligns[0][1][0, 0].tolist() == [ord(c) for c in 'Fraktur '] + [0x1D509, 10]          # ONE symbol per code point
    assert aligns[1][1][1, 1].tolist() == [0x10FFFF] * 2 and aligns[1][3].tolist() == [0, 0, 0]
    assert [c[1:] for c in calls if isinstance(c[0], str) and c[0] == 'vote'] == [(10, None), (2, None), (1, None)]       # C = the chunk's largest ncol, at least 1
    for j, cands in enumerate(CANDIDATES):
        if not cands:
            assert (lines[j], confmats[j], pivots[j], columns[j]) == ('', [], None, [])
            continue
        assert (lines[j], confmats[j], columns[j]) == _direct(cands, pivots[j])
        assert [chunk[0][0] for chunk in confmats[j]] == [col[0][0] for col in columns[j]]      # the first alternative is the best
        assert ''.join(chunk[0][0] for chunk in confmats[j]) == lines[j]
    assert lines[0] == 'Fraktur \U0001D509\n' and confmats[0][8] == [('\U0001D509', 2 / 3), ('\U0001D50A', 1 / 3)]
    assert columns[0][8] == [('\U0001D509', 2.0, [0, 2]), ('\U0001D50A', 1.0, [1])] and confmats[0][0] == [('F', 1.0)]
    assert lines[2] == 'long s: ſ\n' and lines[5] == 'x\n' and confmats[5][0] == [('x', 0.5), ('y', 0.5)]
    assert lines[4] == '\U0010FFFF' and confmats[4] == [[('', 0.5), ('\U0010FFFF', 0.5)], [('\U0010FFFF', 1.0)]]
    assert (lines[6], confmats[6], pivots[6], columns[6]) == ('', [], 0, [])                    # nothing but empty candidates
    # N identical candidates: that line with p = 1; N = 1
    assert s2s.confusion_of([['same\n'] * 5])[:2] == (['same\n'], [[[(c, 1.0)] for c in 'same\n']])
    assert lines[3] == 'a\n' and confmats[3] == [[('a', 1.0)], [('\n', 1.0)]] and columns[3] == [[('a', 1.0, [0])], [('\n', 1.0, [0])]]
    # a result never depends on the chunk: one call for all, one call per source
    for batch_size in (1, 3, 100):
        other = _stub_facade(batch_size)
        assert other.confusion_of(CANDIDATES) == (lines, confmats, pivots, columns)
    assert [c[1].shape for c in other.engine.calls if isinstance(c[0], str) and c[0] == 'align'] == [(6, 5, 10)]
    assert s2s.confusion_of([]) == ([], [], [], []) and s2s.confusion_of([[], []]) == (['', ''], [[], []], [None, None], [[], []])


def test_confusion_of_weights_pivots_and_floor():
    weights = [[1.0, 0.0, 2.5], None, None, [3], [0.5, 0.25], [0.125, 1, 0.25, 0.5], [0, 1]]
    pivots = [1, None, 4, 0, 1, 3, 1]
    s2s = _stub_facade(100)
    lines, confmats, used, columns = s2s.confusion_of(CANDIDATES, weights=weights, pivots=pivots, floor=0.3)
    assert used == pivots and [c[0] for c in s2s.engine.calls] == ['align', 'vote']             # given pivots: no consensus call
    assert s2s.engine.calls[0][3].tolist() == [1, 4, 0, 1, 3, 1]
    assert s2s.engine.calls[1][2].tolist() == [[1.0, 0.0, 2.5, 1.0, 1.0], [1.0] * 5, [3.0, 1.0, 1.0, 1.0, 1.0], [0.5, 0.25, 1.0, 1.0, 1.0],
                                               [0.125, 1.0, 0.25, 0.5, 1.0], [0.0, 1.0, 1.0, 1.0, 1.0]]
    for j, cands in enumerate(CANDIDATES):
        if cands:
            assert (lines[j], confmats[j], columns[j]) == _direct(cands, pivots[j], weights[j], floor=0.3)
    # the floor drops alternatives, never the first; the columns keep them
    assert confmats[0][8] == [('\U0001D509', 1.0)] and columns[0][8] == [('\U0001D509', 3.5, [0, 2]), ('\U0001D50A', 0.0, [1])]
    assert confmats[5][0] == [('y', 1.5 / 1.875)] and len(columns[5][0]) == 2
    assert s2s.confusion_of(CANDIDATES, weights=weights, pivots=pivots, floor=2.0)[1][5][0] == [('y', 1.5 / 1.875)]
    unfloored = s2s.confusion_of(CANDIDATES, weights=weights, pivots=pivots)
    assert unfloored[1][5][0] == [('y', 0.8), ('x', 0.2)] and unfloored[3] == columns and unfloored[0] == lines
    # pivots=None takes consensus_of's picks under the same weights and normalisation
    s2s = _stub_facade(100)
    got = s2s.confusion_of(CANDIDATES, weights=weights, normalise=True)
    assert got[2] == s2s.consensus_of(CANDIDATES, weights=weights, normalise=True)[0]
    assert s2s.engine.calls[0][3] == 1 and s2s.engine.calls[0][2] is not None
    assert _stub_facade(1).confusion_of(CANDIDATES, weights=weights, normalise=True) == got


def test_confusion_of_refuses():
    s2s = _stub_facade(8)
    for bad in (dict(candidates=[['a']], weights=[[1.0], [1.0]]), dict(candidates=[['a', 'b']], weights=[[1.0]]),
                dict(candidates=[['a']], weights=[[-1.0]]), dict(candidates=[['a']], weights=[[math.nan]]),
                dict(candidates=[['a']], weights=[[math.inf]]), dict(candidates=[['a'] * 257]),
                dict(candidates=[['a' * 2049]]), dict(candidates=[[b'a']]), dict(candidates=[[None]]),
                dict(candidates=[['a', 'b']], weights=[[0.0, 0.0]]), dict(candidates=[['a'], ['a', 'b']], weights=[None, [0, 0]]),
                dict(candidates=[['a', 'b']], pivots=[2]), dict(candidates=[['a', 'b']], pivots=[-1]), dict(candidates=[['a', 'b']], pivots=[None]),
                dict(candidates=[['a', 'b']], pivots=[0, 0]), dict(candidates=[['a', 'b']], pivots=[0.0]), dict(candidates=[[], ['a']], pivots=[0, 0])):
        with pytest.raises(ValueError):
            s2s.confusion_of(**bad)
        with pytest.raises(ValueError):
            s2s.correct_candidates(**bad)
    assert s2s.engine.calls == []                             # refused before anything reaches the engine
    lines = s2s.confusion_of([['a'] * 256, ['a' * 2048, 'b']], pivots=[255, np.int64(1)])[0]     # the limits themselves are served
    assert lines == ['a', 'a' * 2048]                         # (equal masses: the lower index, the pivot's gaps included)


class _Corrector(object):
    """correct_lines of a facade, answered in upper case; keeps what it was asked."""

    def __init__(self):
        self.asked = []

    def correct_lines(self, lines, conf=None, fast=True, greedy=True, alignments=True):
        self.asked.append(dict(lines=list(lines), conf=conf, fast=fast, greedy=greedy, alignments=alignments))
        return [line.upper() for line in lines], [[0.5] * len(line) for line in lines], [float(len(line)) for line in lines], [[line] for line in lines]


def test_correct_candidates_assembly():
    sources = [[], ['one\n', 'ome\n', 'one\n'], ['', ''], ['tw\n', 'two\n'], []]          # an empty first source; a network without columns
    s2s = _stub_facade(8, status=2)
    corrector = _Corrector()
    s2s.correct_lines = corrector.correct_lines
    voted, confmats, _, _ = s2s.confusion_of(sources, pivots=[None, 0, 1, 1, None], floor=0.1)
    got = s2s.correct_candidates(sources, pivots=[None, 0, 1, 1, None], floor=0.1, fast=False, greedy=True, alignments='dense')
    assert voted == ['', 'one\n', '', 'tw\n', ''] and confmats[2] == [] and confmats[3][2] == [('', 0.5), ('o', 0.5)]
    assert corrector.asked == [dict(lines=['one\n', 'tw\n'], conf=[confmats[1], confmats[3]], fast=False, greedy=True, alignments='dense')]
    assert got == (['', 'ONE\n', '', 'TW\n', ''], [[], [0.5] * 4, [], [0.5] * 3, []], [0.0, 4.0, 0.0, 3.0, 0.0], [[], ['one\n'], [], ['tw\n'], []])
    assert type(corrector.asked[0]['conf'][0][0]) is list     # (what _sparse_lines reads to tell a network from confidences)
    # nothing to correct: correct_lines is not called at all
    corrector.asked.clear()
    assert s2s.correct_candidates([[], ['']]) == (['', ''], [[], []], [0.0, 0.0], [[], []]) and corrector.asked == []
    assert s2s.correct_candidates([]) == ([], [], [], [])


def test_the_networks_are_what_the_model_s_input_stage_reads():
    """`_sparse_lines` on a voted network: one position per column, the alternatives' indices and probabilities, '' contributing
    nothing, characters outside the mapping behaving as anywhere else (index 0)."""
    s2s = _stub_facade(8)
    s2s.mapping = ({'': 0, '\n': 1, 'a': 2, 'b': 3}, {0: '', 1: '\n', 2: 'a', 3: 'b'})
    s2s.voc_size = 4
    _, confmats, _, _ = s2s.confusion_of([['ab\n', 'b\n', 'aa\n', 'aſ\n']], pivots=[0])
    assert confmats[0] == [[('a', 0.75), ('', 0.25)], [('b', 0.5), ('a', 0.25), ('ſ', 0.25)], [('\n', 1.0)]]
    idx, val, _ = s2s._sparse_lines(['ab\n'], confmats)
    assert idx.shape == (1, 3, 3) and idx[0].tolist() == [[2, -1, -1], [3, 2, 0], [1, -1, -1]]
    assert val[0].tolist() == [[0.75, 0, 0], [0.5, 0.25, 0.25], [1.0, 0, 0]]


# ------------------------------------------------------------------------------------------------------------------ 4. the binding
def test_the_entries_are_bound():
    from ctypes import c_int, c_int32, c_int64, c_void_p
    from cor_asv_ann_amd import _native as nv
    assert nv.SIGNATURES['casv_consensus_align'] == (c_int, [c_void_p, c_int32, c_int32, c_int32] + [c_void_p] * 5)
    assert nv.SIGNATURES['casv_consensus_vote'] == (c_int, [c_void_p, c_int32] + [c_void_p] * 4)
    assert nv.SIGNATURES['casv_debug_set_align_budget'] == (c_int, [c_void_p, c_int64])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'cor_asv_ann_hip.h')) as f:
        header = f.read()
    assert 'int casv_consensus_align(casv_model* m, int32_t B, int32_t N, int32_t L,' in header
    assert 'int casv_consensus_vote(casv_model* m, int32_t C, const double* weight,' in header
    assert 'int casv_debug_set_align_budget(casv_model* m, int64_t bytes);' in header and '#define CASV_ALIGN_NONE INT32_MIN' in header
    with open(os.path.join(root, 'cor_asv_ann_amd', 'csrc', 'Makefile')) as f:
        assert ' consensus_align.hip' in f.read()
    with open(os.path.join(root, 'cor_asv_ann_amd', 'csrc', 'common.h')) as f:
        assert 'CONSENSUS_ALIGN_MAX_L = %d' % ac.MAX_L in f.read()
    from cor_asv_ann_amd.engine import HipEngine
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence
    assert all(hasattr(HipEngine, name) for name in ('consensus_align', 'consensus_vote', 'debug_set_align_budget'))
    assert all(hasattr(Sequence2Sequence, name) for name in ('confusion_of', 'correct_candidates'))
    lib = nv.load()
    assert all(hasattr(lib, name) for name in ('casv_consensus_align', 'casv_consensus_vote', 'casv_debug_set_align_budget'))
