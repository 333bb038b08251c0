"""tests/consensus_cases.py held on the CPU: the restated edit distance against the project's own and against known answers, the
rules of risk and pick, the case list the device runs, and the facade (consensus_of, consensus_lines) on a stub engine that answers
from the restatement.  The device's side: tests/test_gpu_consensus.py."""
import math
import os

import numpy as np
import pytest

from tests import consensus_cases as cc


def _points(text):
    return np.array([ord(c) for c in text], np.int32)


# ------------------------------------------------------------------------------------------------------------------ 1. the distance
def test_known_answers():
    assert cc.levenshtein(_points('kitten'), _points('sitting')) == 3
    assert cc.levenshtein(_points('sitting'), _points('kitten')) == 3
    assert cc.levenshtein(_points('flaw'), _points('lawn')) == 2
    for n in (0, 1, 7, 200):
        s = np.arange(n, dtype=np.int32)
        assert cc.levenshtein(s[:0], s) == n and cc.levenshtein(s, s[:0]) == n
        assert cc.levenshtein(s, s.copy()) == 0
    assert cc.levenshtein([cc.I32_MAX], [cc.I32_MIN]) == 1 and cc.levenshtein([0x10FFFF, -1], [0x10FFFF, -1]) == 0


def test_against_the_project_s_own_distance():
    from cor_asv_ann_amd.metrics import Alignment
    rng = np.random.default_rng(1)
    for trial in range(150):
        alphabet = [[3], [0, 1], list(range(30))][trial % 3]
        a = cc._draw(rng, alphabet, int(rng.integers(0, 40)))
        b = cc._mutate(rng, a, alphabet, int(rng.integers(0, 12))) if trial % 2 else cc._draw(rng, alphabet, int(rng.integers(0, 40)))
        want, longer = Alignment.get_levenshtein_distance(a.tolist(), b.tolist())
        assert cc.levenshtein(a, b) == want and longer == max(len(a), len(b))


def test_symmetry_and_triangle_inequality():
    rng = np.random.default_rng(2)
    for trial in range(100):
        alphabet = [[0, 1], [0, 1, 2, 3]][trial % 2]
        x, y, z = (cc._draw(rng, alphabet, int(rng.integers(0, 30))) for _ in range(3))
        xy, yz, xz = cc.levenshtein(x, y), cc.levenshtein(y, z), cc.levenshtein(x, z)
        assert xy == cc.levenshtein(y, x)
        assert xz <= xy + yz
        assert abs(len(x) - len(y)) <= xy <= max(len(x), len(y))


# ------------------------------------------------------------------------------------------------------------------ 2. risk and pick
def test_risk_and_pick_rules():
    sym, length = cc.pack([_points('abcd'), _points('abed'), None, _points('abcd'), _points('xy')])
    D = cc.distance_matrix(sym, length)
    assert D.tolist() == [[0, 1, -1, 0, 4], [1, 0, -1, 1, 4], [-1] * 5, [0, 1, -1, 0, 4], [4, 4, -1, 4, 0]]
    risk, pick = cc.risk_and_pick(D, length)
    assert risk.tolist() == [5.0, 6.0, math.inf, 5.0, 12.0] and pick == 0                  # duplicates tie: the lower index
    risk, pick = cc.risk_and_pick(D, length, [0.0, 0.0, 9.0, 0.0, 2.0])
    assert risk.tolist() == [8.0, 8.0, math.inf, 8.0, 0.0] and pick == 4                   # (a padding candidate's weight is not read)
    risk, pick = cc.risk_and_pick(D, length, mode=1)
    assert risk.tolist() == [0.25 + 1.0, 0.25 + 0.25 + 1.0, math.inf, 0.25 + 1.0, 3.0] and pick == 0
    risk, pick = cc.risk_and_pick(D, length, [0.0] * 5)
    assert risk.tolist() == [0.0, 0.0, math.inf, 0.0, 0.0] and pick == 0
    sym, length = cc.pack([None, None])
    risk, pick = cc.risk_and_pick(cc.distance_matrix(sym, length), length)
    assert risk.tolist() == [math.inf, math.inf] and pick == -1
    sym, length = cc.pack([_points(''), None, _points('')])                                # two empty lines: distance 0, divided by 1
    assert cc.risk_and_pick(cc.distance_matrix(sym, length), length, mode=1)[0].tolist() == [0.0, math.inf, 0.0]
    # the order of the sum is the candidates' order: 2^53 + 1 + 1 is not 1 + 1 + 2^53
    sym, length = cc.pack([[1], [2], [3], []])
    D = np.array([[0, 1, 1, 1]] * 4)
    assert cc.risk_and_pick(D, length, [0.0, 2.0 ** 53, 1.0, 1.0])[0][0] == 2.0 ** 53
    assert cc.risk_and_pick(D, length, [0.0, 1.0, 1.0, 2.0 ** 53])[0][0] == 2.0 ** 53 + 2.0


def test_the_case_list_is_the_issue_s():
    cases = {c[0]: c for c in cc.cases()}
    assert len(cases) == len(cc.cases())
    for name in ('one', 'two', 'many'):
        assert cases['lengths_' + name][2].tolist() == [[0, 1, 2, 63, 64, 65, 127, 128, 129, 200]]
        assert len(np.unique(cases['lengths_' + name][1])) <= max(len(cc.ALPHABETS[name]), 2)
    many = set(cases['lengths_many'][1].ravel().tolist())
    assert {0, 0x10FFFF, cc.I32_MAX}.issubset(many) and min(many) < 0
    assert cases['pair_700_650'][2].tolist() == [[700, 650]] and cases['pair_8192_1'][2].tolist() == [[8192, 1]]
    assert sorted(c[1].shape[1] for c in cases.values() if c[0].startswith('shape_N') and 'padding' not in c[0]) == [1, 2, 3, 64, 65, 256]
    assert sorted(c[1].shape[0] for c in cases.values() if c[0].endswith('_padding')) == [1, 3, 70]
    lots = cases['sources_%d' % cc.MANY_SOURCES]
    assert lots[1].shape[0] == cc.MANY_SOURCES > 65535 and len({(s.tobytes(), l.tobytes()) for s, l in zip(lots[1][:2000], lots[2][:2000])}) > 40
    length = np.concatenate([c[2] for c in cases.values() if c[0].endswith('_padding')])
    assert (length[:, 0] < 0).any() and (length[:, 2] < 0).any() and (length[:, 4] < 0).any() and (length < 0).all(axis=1).any()
    for c in cc.cases():
        name, sym, length, w, mode = c
        assert sym.dtype == np.int32 and length.dtype == np.int32 and sym.shape[:2] == length.shape and mode in (0, 1)
        assert 1 <= sym.shape[1] <= cc.MAX_N and sym.shape[2] <= cc.MAX_L and length.min() >= -1 and length.max() <= sym.shape[2]
        assert w is None or (w.shape == length.shape and w.dtype == np.float64 and np.isfinite(w).all() and (w >= 0).all())
    w = cases['weights_mode0'][3]
    assert (w == 0).any() and np.log10(w[w > 0].max()) - np.log10(w[w > 0].min()) > 100
    risk, pick, dist = cc.expected('ties_mode0')
    assert risk[0, 0] == risk[0, 3] and risk[0, 1] == risk[0, 2] and pick[0] == int(np.argmin(risk[0])) and pick[2] in (1, 2)
    assert (dist[2, 0] == -1).all() and risk[2, 0] == math.inf
    risk, pick, _ = cc.expected('all_weights_zero')
    assert (risk == 0).all() and pick.tolist() == [0, 0]
    risk, pick, dist = cc.expected('shape_N5_B70_padding')
    empty = (cases['shape_N5_B70_padding'][2] < 0).all(axis=1)
    assert empty.any() and (pick[empty] == -1).all() and np.isinf(risk[empty]).all() and (dist[empty] == -1).all()
    assert (pick[~empty] >= 0).all()


def test_poison_leaves_the_live_symbols_alone():
    _, sym, length, _, _ = cc.cases()[cc.CASE_IDS.index('weights_mode0')]
    for how in ('other', 'random'):
        p = cc.poisoned(sym, length, how)
        assert not np.array_equal(p, sym)
        for b in range(sym.shape[0]):
            for i in range(sym.shape[1]):
                n = max(int(length[b, i]), 0)
                assert np.array_equal(p[b, i, :n], sym[b, i, :n])
        assert cc.same(cc.reference(p, length), cc.reference(sym, length))


# ------------------------------------------------------------------------------------------------------------------ 3. the facade
def _stub_facade(batch_size, status=0):
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence
    s2s = Sequence2Sequence()
    s2s.batch_size = batch_size
    s2s.engine = cc.StubEngine()
    s2s.status = status
    return s2s


# (outside the Basic Multilingual Plane, and characters no mapping of the tests has)
CANDIDATES = [['Fraktur \U0001D509\n', 'Fraktur \U0001D50A\n', 'Fraktur \U0001D509\n'],
              [],
              ['long s: ſ\n', '', 'long s: s\n', 'long ſ: s\n', 'lonɡ s: ſ\n'],
              ['a\n'],
              ['\U0010FFFF', '\U0010FFFF\U0010FFFF'],
              ['x\n', 'y\n', 'x\n', 'y\n']]


def _direct(cands, weights=None, mode=0):
    sym, length = cc.pack([_points(c) for c in cands])
    D = cc.distance_matrix(sym, length)
    risk, pick = cc.risk_and_pick(D, length, weights, mode)
    return pick, risk.tolist(), D.tolist()


def test_consensus_of_chunks_pads_and_converts():
    s2s = _stub_facade(12)                                    # works on an empty model: status 0, no vocabulary
    picks, risks, dists = s2s.consensus_of(CANDIDATES, distances=True)
    calls = s2s.engine.calls
    # chunks as score_candidates': sources x the largest count within max(batch_size, count) rows -- [0, 2], [3, 4, 5]; [1] has none
    assert [c[0].shape for c in calls] == [(2, 5, 10), (3, 4, 2)]
    assert calls[0][1].tolist() == [[10, 10, 10, -1, -1], [10, 0, 10, 10, 10]]                  # padding candidates: -1
    assert calls[1][1].tolist() == [[2, -1, -1, -1], [1, 2, -1, -1], [2, 2, 2, 2]]
    assert calls[0][0][0, 0].tolist() == [ord(c) for c in 'Fraktur '] + [0x1D509, 10]           # ONE symbol per code point
    assert calls[0][0][1, 4, 3] == 0x261 and calls[1][0][1, 1].tolist() == [0x10FFFF] * 2
    assert all(c[2] is None and c[3] == 0 and c[4] is True for c in calls)
    for j, cands in enumerate(CANDIDATES):
        if not cands:
            assert picks[j] is None and risks[j] == [] and dists[j] == []
            continue
        pick, risk, D = _direct(cands)
        assert (picks[j], risks[j], dists[j]) == (pick, risk, D) and isinstance(picks[j], int)
    assert picks == [0, None, 0, 0, 0, 0] and dists[0] == [[0, 1, 0], [1, 0, 1], [0, 1, 0]] and risks[5] == [2.0] * 4
    # a result never depends on the chunk: one call for all, one call per source
    for batch_size in (1, 3, 100):
        other = _stub_facade(batch_size)
        assert other.consensus_of(CANDIDATES, distances=True) == (picks, risks, dists)
    assert [c[0].shape for c in other.engine.calls] == [(5, 5, 10)]
    assert s2s.consensus_of(CANDIDATES)[2] == [[] for _ in CANDIDATES]
    assert s2s.consensus_of([]) == ([], [], []) and s2s.consensus_of([[], []]) == ([None, None], [[], []], [[], []])


def test_consensus_of_weights_and_normalise():
    weights = [[1.0, 0.0, 2.5], None, None, [3], [0.5, 0.25], [0, 0, 0, 0]]
    s2s = _stub_facade(100)
    picks, risks, _ = s2s.consensus_of(CANDIDATES, weights=weights, normalise=True)
    sym, length, w, mode, want_dist = s2s.engine.calls[0]
    assert mode == 1 and want_dist is False
    assert w.tolist() == [[1.0, 0.0, 2.5, 1.0, 1.0], [1.0] * 5, [3.0, 1.0, 1.0, 1.0, 1.0], [0.5, 0.25, 1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0, 1.0]]
    for j, cands in enumerate(CANDIDATES):
        if cands:
            pick, risk, _ = _direct(cands, weights[j], 1)
            assert (picks[j], risks[j]) == (pick, risk)
    assert picks[5] == 0 and risks[5] == [0.0] * 4
    separate = _stub_facade(1).consensus_of(CANDIDATES, weights=weights, normalise=True)
    assert separate[:2] == (picks, risks)


def test_consensus_of_refuses():
    s2s = _stub_facade(8)
    for bad in (dict(candidates=[['a']], weights=[[1.0], [1.0]]), dict(candidates=[['a', 'b']], weights=[[1.0]]),
                dict(candidates=[['a']], weights=[[-1.0]]), dict(candidates=[['a']], weights=[[math.nan]]),
                dict(candidates=[['a']], weights=[[math.inf]]), dict(candidates=[['a'] * 257]),
                dict(candidates=[['a' * 8193]]), dict(candidates=[[b'a']]), dict(candidates=[[None]])):
        with pytest.raises(ValueError):
            s2s.consensus_of(**bad)
    assert s2s.engine.calls == []                             # refused before anything reaches the engine
    s2s.consensus_of([['a'] * 256, ['a' * 8192]])             # the limits themselves are served


class _Sampler(object):
    """sample_lines / correct_lines of a facade, answered from a table; keeps what it was asked."""
    TABLE = {'one\n': ['ome\n', 'one\n', 'onc\n'], 'two\n': ['two\n', 'tvvo\n', 'tw0\n'], 'three\n': ['tree\n', 'thre\n', 'there\n']}

    def __init__(self):
        self.asked = []

    def sample_lines(self, lines, conf=None, n=1, temperature=1.0, top_k=0, seed=None, streams=None, alignments=False, top_p=1.0):
        self.asked.append(dict(lines=list(lines), conf=conf, n=n, temperature=temperature, top_k=top_k, seed=seed, streams=streams,
                               alignments=alignments, top_p=top_p))
        cands = [self.TABLE[line][:n] if line else [] for line in lines]
        # log p - log q per character: candidate k of a line sums to -(k + 1) * 0.5 * its length
        logp = [[[-1.0 - 0.5 * k] * len(c) for k, c in enumerate(cs)] for cs in cands]
        logq = [[[-1.0] * len(c) for c in cs] for cs in cands]
        return cands, logp, [[1.0] * len(cs) for cs in cands], logq, [[[] for _ in cs] for cs in cands]

    def correct_lines(self, lines, conf=None, fast=True, greedy=True, alignments=True):
        self.asked.append(dict(lines=list(lines), conf=conf, fast=fast, greedy=greedy, alignments=alignments))
        return [line.upper() for line in lines], [[1.0] * len(line) for line in lines], [0.0] * len(lines), [[] for _ in lines]


def _sampling_facade():
    s2s = _stub_facade(8, status=2)
    sampler = _Sampler()
    s2s.sample_lines, s2s.correct_lines = sampler.sample_lines, sampler.correct_lines
    return s2s, sampler


LINES = ['one\n', '', 'two\n', 'three\n']


def test_consensus_lines_assembly():
    s2s, sampler = _sampling_facade()
    conf = [None] * 4
    lines, risks, cands, picks = s2s.consensus_lines(LINES, conf=conf, n=3, temperature=0.7, top_k=5, top_p=0.9, seed=11, streams=[4, 5, 6, 7])
    assert sampler.asked[0] == dict(lines=LINES, conf=conf, n=3, temperature=0.7, top_k=5, seed=11, streams=[4, 5, 6, 7], alignments=False, top_p=0.9)
    assert sampler.asked[1] == dict(lines=LINES, conf=conf, fast=True, greedy=True, alignments=False)
    assert cands == [['ONE\n'] + _Sampler.TABLE['one\n'], [], ['TWO\n'] + _Sampler.TABLE['two\n'], ['THREE\n'] + _Sampler.TABLE['three\n']]
    assert (lines[1], risks[1], cands[1], picks[1]) == ('', 0.0, [], None)                  # the empty source
    for j in (0, 2, 3):
        pick, risk, _ = _direct(cands[j])
        assert picks[j] == pick and lines[j] == cands[j][pick] and risks[j] == risk[pick] and isinstance(risks[j], float)
    assert s2s.engine.calls[0][2] is None and s2s.engine.calls[0][3] == 0                    # uniform: no weights, mode 0
    # without the greedy line: the samples alone, and no greedy decode
    s2s, sampler = _sampling_facade()
    lines, risks, cands, picks = s2s.consensus_lines(LINES, n=2, seed=1, include_greedy=False, normalise=True)
    assert len(sampler.asked) == 1 and cands == [_Sampler.TABLE['one\n'][:2], [], _Sampler.TABLE['two\n'][:2], _Sampler.TABLE['three\n'][:2]]
    assert s2s.engine.calls[0][3] == 1 and picks == [0, None, 0, 0]
    assert _sampling_facade()[0].consensus_lines([]) == ([], [], [], [])
    assert _sampling_facade()[0].consensus_lines(['']) == ([''], [0.0], [[]], [None])
    with pytest.raises(ValueError):
        s2s.consensus_lines(LINES, weights='likelihood')


def test_consensus_lines_importance_weights():
    def expect(text_lengths, greedy):
        s = []
        for k, n in enumerate(text_lengths):
            total = 0.0
            for _ in range(n):
                total = total + ((-1.0 - 0.5 * k) - (-1.0))
            s.append(total)
        e = [math.exp(x - max(s)) for x in s]
        z = 0.0
        for x in e:
            z = z + x
        w = [x / z for x in e]
        mean = 0.0
        for x in w:
            mean = mean + x
        return ([mean / len(w)] if greedy else []) + w

    for greedy in (True, False):
        s2s, _ = _sampling_facade()
        lines, risks, cands, picks = s2s.consensus_lines(LINES, n=3, seed=2, weights='importance', include_greedy=greedy)
        w = np.concatenate([c[2] for c in s2s.engine.calls])
        live = [j for j, line in enumerate(LINES) if line]
        assert w.shape == (3, 4 if greedy else 3)
        for b, j in enumerate(live):
            want = expect([len(c) for c in _Sampler.TABLE[LINES[j]]], greedy)
            assert w[b].tolist() == want                                                    # bit for bit: float64 on the host, in order
            assert sum(want[1:] if greedy else want) == pytest.approx(1.0, abs=1e-15)
            pick, risk, _ = _direct(cands[j], want)
            assert picks[j] == pick and risks[j] == risk[pick]
        assert lines[1] == '' and picks[1] is None


# ------------------------------------------------------------------------------------------------------------------ 4. the binding
def test_the_entry_is_bound():
    from ctypes import c_int, c_int32, c_void_p
    from cor_asv_ann_amd import _native as nv
    assert nv.SIGNATURES['casv_consensus'] == (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32] + [c_void_p] * 6)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'cor_asv_ann_hip.h')) as f:
        header = f.read()
    assert 'int casv_consensus(casv_model* m, int32_t B, int32_t N, int32_t L, int32_t mode,' in header
    with open(os.path.join(root, 'cor_asv_ann_amd', 'csrc', 'Makefile')) as f:
        assert ' consensus_kernels.hip ' in f.read()
    assert hasattr(nv.load(), 'casv_consensus')
