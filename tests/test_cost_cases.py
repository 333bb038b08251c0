"""tests/cost_cases.py held on the CPU: the costed restatement against the unit-cost ones and against answers made by hand, its
symmetries, the case list the device runs -- with the condition that every wrong variant differs from the definition on one of
its cases, which keeps tests/test_gpu_costed_consensus.py from being vacuous -- and the facade (EditCosts, consensus_of,
confusion_of, correct_candidates, consensus_lines, risk_candidates) on a stub engine that answers from the restatement."""
import numpy as np
import pytest

from tests import align_cases as ac
from tests import consensus_cases as cc
from tests import cost_cases as k


def _points(text):
    return np.array([ord(c) for c in text], np.int32)


def _pairs(name):
    """The (pivot, candidate) pairs of a case as (p, kp, c, kc), every pair once."""
    sym, key, length, pivot, _, _, _ = k.case(name)[:7]
    seen = set()
    for b in range(len(pivot)):
        if pivot[b] < 0:
            continue
        for c in range(length.shape[1]):
            if length[b, c] < 0 or c == pivot[b]:
                continue
            p, kp = k._live(sym[b], None if key is None else key[b], length[b], int(pivot[b]))
            q, kq = k._live(sym[b], None if key is None else key[b], length[b], c)
            mark = (p.tobytes(), q.tobytes(), None if kp is None else kp.tobytes() + kq.tobytes())
            if mark not in seen:
                seen.add(mark)
                yield p, kp, q, kq


# ------------------------------------------------------------------------------------------------------------------ 1. the definition
def test_answers_made_by_hand():
    s, f = _points('s'), _points('ſ')
    one = np.array([7], np.int32)
    # two different symbols: sub without keys and under different keys, near under equal keys; equal symbols cost 0 whatever the keys
    assert k.distance(s, None, f, None, (2, 3, 1, 3)) == 3
    assert k.distance(s, one, f, one + 1, (2, 3, 1, 3)) == 3 and k.distance(s, one, f, one, (2, 3, 1, 3)) == 1
    assert k.distance(s, one, s, one + 1, (2, 3, 1, 3)) == 0 and k.distance(s, one, s, one, (2, 3, 1, 3)) == 0
    # a substitution that never beats two indels: (1, 3, 0)
    assert k.distance(_points('ab'), None, _points('ac'), None, (1, 3, 0, 3)) == 2
    assert k.walk(_points('ab'), None, _points('ac'), None, (1, 3, 0, 3)).tolist() == [0, -2]       # c in front of b, which stands against a gap
    # borders and empty strings: n * gap
    assert k.matrix(_points('abc'), None, _points('xy'), None, (5, 9, 9, 1))[:, 0].tolist() == [0, 5, 10, 15]
    assert k.distance(_points(''), None, _points('abcd'), None, (5, 9, 9, 1)) == 20 == k.distance(_points('abcd'), None, _points(''), None, (5, 9, 9, 1))
    # kitten / sitting at gap 2, sub 3: k/s and e/i cost 3 each, the g 2
    assert k.distance(_points('kitten'), None, _points('sitting'), None, (2, 3, 3, 3)) == 8
    # near pairs draw two readings into one column: 'is' against 'iſt' puts ſ on s under the keys, and ſ and t in front of s without them at (1,3,0)
    hl = np.array([0, 1], np.int32), np.array([0, 1, 2], np.int32)
    assert k.walk(_points('is'), hl[0], _points('iſt'), hl[1], (1, 3, 0, 3)).tolist() == [0, 1, -3]
    assert k.walk(_points('is'), None, _points('iſt'), None, (1, 3, 0, 3)).tolist() == [0, -2, -2]


def test_unit_costs_are_the_plain_restatements():
    """Costs (1, 1, 1) with or without keys reproduce consensus_cases.levenshtein and align_cases.walk on every case."""
    done = set()        # (the cases of one alphabet share their strings)
    for name in k.CASE_IDS:
        for p, kp, c, kc in _pairs(name):
            mark = (p.tobytes(), c.tobytes(), None if kp is None else kp.tobytes() + kc.tobytes())
            if mark in done:
                continue
            done.add(mark)
            for keys in ((kp, kc), (None, None)):
                assert k.distance(p, keys[0], c, keys[1], k.UNIT) == cc.levenshtein(p, c)
                assert np.array_equal(k.walk(p, keys[0], c, keys[1], k.UNIT), ac.walk(p, c)[0])


def test_no_keys_is_keys_equal_to_symbols_is_near_equal_to_sub():
    for name in ('lengths_four_2_3_1_u3', 'lengths_three_2_3_1_u3', 'odd_symbols_and_keys', 'asymmetric_3_65'):
        for p, kp, c, kc in _pairs(name):
            want = k.distance(p, None, c, None, (2, 3, 1, 3)), k.walk(p, None, c, None, (2, 3, 1, 3))
            for keys, costs in (((p, c), (2, 3, 1, 3)), ((kp, kc), (2, 3, 3, 3))):
                assert k.distance(p, keys[0], c, keys[1], costs) == want[0]
                assert np.array_equal(k.walk(p, keys[0], c, keys[1], costs), want[1])


def test_the_matrix_is_symmetric():
    for name in ('lengths_four_2_3_1_u3', 'lengths_two_1_1_0_u1', 'lengths_four_keys_per_position', 'odd_symbols_and_keys'):
        costs = k.case(name)[6]
        for p, kp, c, kc in _pairs(name):
            assert np.array_equal(k.matrix(p, kp, c, kc, costs), k.matrix(c, kc, p, kp, costs).T)
        dist = k.expected(name)[2]
        assert np.array_equal(dist, dist.transpose(0, 2, 1))


def test_the_walk_s_cost_is_the_distance():
    """Read off `where` alone: the substitutions under the costs, gap per pivot symbol without a partner and per insertion."""
    for name in ('lengths_four_2_3_1_u3', 'lengths_four_1_3_0_u3', 'lengths_two_1_1_0_u1', 'odd_symbols_and_keys'):
        costs = k.case(name)[6]
        for p, kp, c, kc in _pairs(name):
            where = k.walk(p, kp, c, kc, costs)
            hit = where >= 0
            subs = sum(int(k.sub_cost(p[i], kp[i], c[j:j + 1], kc[j:j + 1], costs)[0]) for j, i in enumerate(where) if i >= 0)
            assert subs + costs[0] * ((len(p) - int(hit.sum())) + int((~hit).sum())) == k.distance(p, kp, c, kc, costs)
            assert (np.diff(where[hit]) > 0).all()


# ------------------------------------------------------------------------------------------------------------------ 2. the case list
def test_the_case_list_is_the_issue_s():
    cases = {c[0]: c for c in k.cases()}
    assert len(cases) == len(k.cases())
    assert k.LENGTHS == [0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200]
    for name, alphabet in k.ALPHABETS.items():
        _, sym, key, length, pivot, _, _, _ = cases['lengths_%s_2_3_1_u3' % name]
        assert 2 <= len(alphabet) <= 4 and sorted(length[0].tolist()) == k.LENGTHS and pivot.tolist() == list(range(len(k.LENGTHS)))
        assert np.array_equal(key, np.mod(sym, 2)) and set(np.unique(sym[0, -1])) == set(alphabet)
    have = {c[7] for c in k.cases()}
    assert have >= {(1, 1, 1, 1), (1, 1, 0, 1), (2, 2, 1, 2), (2, 3, 1, 3), (1, 3, 0, 3), (255, 255, 255, 255), (1, 1, 1, 3)}
    assert cases['pair_2048_max_costs'][3].tolist() == [[2048, 2048]] and cases['pair_2048_max_costs'][7] == (255,) * 4
    assert cases['asymmetric_3_65'][3].tolist() == [[3, 65], [65, 3]]
    for N in (1, 2, 3, 64, 65, 256):
        c = next(c for c in k.cases() if c[0].startswith('shape_N%d_' % N))
        assert c[1].shape[1] == N
    assert (cases['shape_N256_B3'][3] < 0).any() and (cases['shape_N3_B2'][4] == -1).any()
    assert cases['sources_66000'][1].shape[0] > 65535
    assert cases['lengths_four_no_keys'][2] is None
    odd = cases['odd_symbols_and_keys']
    assert set(np.unique(odd[1])) <= set(cc.ODD_SYMBOLS) and set(np.unique(odd[2])) <= set(cc.ODD_SYMBOLS) and len(np.unique(odd[2])) >= 4
    assert {c[6] for c in k.cases()} == {0, 1} and any(c[5] is not None for c in k.cases())
    for c in k.cases():
        assert c[1].shape[2] <= k.MAX_L and c[1].shape[1] <= k.MAX_N and (c[2] is None or c[2].shape == c[1].shape)


SMALL = [n for n in k.CASE_IDS if not n.startswith(('pair_2048', 'sources_', 'shape_N256'))]


@pytest.mark.parametrize('variant', k.VARIANTS)
def test_every_wrong_variant_differs_on_a_case_of_the_list(variant):
    """... and on which output: the distance-side variants in dist / risk, the path-side ones in where."""
    hit = next((name for name in SMALL if not k.same(k.reference(*k.case(name), variant=variant), k.expected(name))), None)
    assert hit is not None, variant
    got, want = k.reference(*k.case(hit), variant=variant), k.expected(hit)
    differs = [what for what, g, w in zip(('risk', 'pick', 'dist', 'where', 'ncol', 'src', 'mass', 'best'), got, want) if not k.same((g,), (w,))]
    side = {'unit_ignored': 'risk', 'empty_no_gap': 'dist', 'gap_bit_plus_1': 'where', 'diag_bit_unit': 'where', 'up_first': 'where'}
    assert side.get(variant, differs[0]) in differs


def test_the_variants_leave_the_definition_alone_where_they_should():
    """A variant is a change of one rule: at unit costs without keys all but up_first are the definition."""
    sym, key, length, pivot, w, mode, _ = k.case('lengths_four_1_1_1_u1')
    for variant in k.VARIANTS:
        equal = k.same(k.reference(sym, None, length, pivot, w, mode, k.UNIT, variant=variant), k.reference(sym, None, length, pivot, w, mode, k.UNIT))
        assert equal == (variant != 'up_first'), variant


def test_poison_leaves_the_results_alone():
    name = 'weights_mode1'
    sym, key, length, pivot, w, mode, costs = k.case(name)
    p_sym, p_key = k.poisoned(sym, key, length)
    assert not np.array_equal(p_sym, sym) and not np.array_equal(p_key, key)
    assert k.same(k.reference(p_sym, p_key, length, pivot, w, mode, costs), k.expected(name))


# ------------------------------------------------------------------------------------------------------------------ 3. the facade
def _stub_facade(batch_size, status=0):
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence
    s2s = Sequence2Sequence()
    s2s.batch_size = batch_size
    s2s.engine = k.StubEngine()
    s2s.status = status
    return s2s


# INTEGRATION.md's example: three engines' readings of one Fraktur line -- long s kept, long s modernised, and one that keeps half
# of them and drops the t of "iſt"
READINGS = ['Waſſer iſt ſelten', 'Wasser ist selten', 'Waſſer is selten']


def test_edit_costs_checks_its_values():
    from cor_asv_ann_amd.edit_costs import EditCosts
    assert EditCosts().as_tuple() == (1, 1, 1, 1) and EditCosts(2, 3, 1).as_tuple() == (2, 3, 1, 3)       # unit: sub
    assert EditCosts(2, 3, 1, unit=2).as_tuple() == (2, 3, 1, 2) and EditCosts(1, 0, 0, unit=1).as_tuple() == (1, 0, 0, 1)
    assert EditCosts(255, 255, 255).as_tuple() == (255,) * 4
    for bad in (dict(gap=0), dict(gap=256), dict(sub=256), dict(sub=-1), dict(sub=2, near=3), dict(near=-1), dict(unit=0), dict(unit=256),
                dict(sub=0, near=0), dict(gap=1.5), dict(gap=True), dict(key=3), dict(key='s')):
        with pytest.raises(ValueError):
            EditCosts(**bad)


def test_the_presets_keys():
    from cor_asv_ann_amd import metrics
    from cor_asv_ann_amd.edit_costs import EditCosts
    hl, graded = EditCosts.historic_latin(), EditCosts.graded()
    assert hl.as_tuple() == (1, 1, 0, 1) and graded.as_tuple() == (2, 2, 1, 2)
    key = lambda costs, char: costs.key_of(ord(char))
    for a, b in (('ſ', 's'), ('ꝛ', 'r'), ('ʒ', 'z'), ('—', '-'), ('‐', '–'), ('„', '»'), ('’', "'"), ('µ', 'μ')):
        assert any(a in members and b in members for members in metrics.L1_EQUIVALENCES)
        assert key(hl, a) == key(hl, b)
    assert key(hl, 'ſ') == 's' and key(hl, '—') == '-' and key(hl, 'x') == 'x' and key(hl, 'ä') == 'ä'      # the lowest member; itself
    assert key(hl, 'ſ') != key(hl, 'f') and key(hl, 's') != key(hl, 'S') and key(hl, '„') != key(hl, '“')
    assert key(graded, 'A') == key(graded, 'a') == key(graded, 'ä') == key(graded, 'Ä') == 'a' and key(graded, 'ſ') == key(graded, 's')
    assert key(graded, 'ß') == 'ß' and key(graded, 'a') != key(graded, 'b') and key(graded, '\ud800') == '\ud800'
    # keys_of: dense ids per call in the nesting of the points, None without a key
    points = [[_points('Waſs'), _points('')], [], [_points('sx')]]
    ids = hl.keys_of(points)
    assert [[a.tolist() for a in src] for src in ids] == [[[0, 1, 2, 2], []], [], [[2, 3]]] and all(a.dtype == np.int32 for src in ids for a in src)
    assert EditCosts(2, 2, 1).keys_of(points) is None
    # a dict: code point -> int, a code point it lacks apart from every value; a callable: asked once per code point
    by_dict = EditCosts(2, 2, 1, key={ord('a'): 5, ord('b'): 5, ord('c'): ord('d')})
    assert [a.tolist() for a in by_dict.keys_of([[_points('abcd')]])[0]] == [[0, 0, 1, 2]]
    asked = []
    by_call = EditCosts(2, 2, 1, key=lambda char: asked.append(char) or char.lower())
    by_call.keys_of([[_points('aAbA'), _points('Bab')]])
    by_call.keys_of([[_points('aB')]])
    assert sorted(asked) == ['A', 'B', 'a', 'b']


def test_costs_none_makes_today_s_calls():
    s2s, plain = _stub_facade(8), _stub_facade(8)
    plain.engine = ac.StubEngine()
    cands = [READINGS, [], ['a', 'b']]
    for run in (lambda m: m.consensus_of(cands, weights=[[1, 2, 3], None, None], normalise=True, distances=True),
                lambda m: m.confusion_of(cands, floor=0.1), lambda m: m.confusion_of(cands, pivots=[1, None, 0])):
        assert run(s2s) == run(plain)
    assert len(s2s.engine.calls) == len(plain.engine.calls) > 0
    for mine, theirs in zip(s2s.engine.calls, plain.engine.calls):      # no 'costed' record, the same arguments
        assert len(mine) == len(theirs) and all(type(x) is type(y) and np.array_equal(x, y) for x, y in zip(mine, theirs))


def test_the_facade_passes_costs_and_keys_through():
    from cor_asv_ann_amd.edit_costs import EditCosts
    s2s = _stub_facade(8)
    hl = EditCosts.historic_latin()
    picks, risks, dists = s2s.consensus_of([READINGS, [], ['a', 'b']], normalise=True, distances=True, costs=hl)
    (what, sym, key, length, w, mode, want_dist, costs), = s2s.engine.calls
    assert what == 'costed' and costs == (1, 1, 0, 1) and mode == 1 and want_dist and w is None
    assert sym.shape == key.shape == (2, 3, 17) and length.tolist() == [[17, 17, 16], [1, 1, -1]]
    assert ''.join(map(chr, sym[0, 0])) == READINGS[0] and key[0, 0, 2] == key[0, 1, 2] and sym[0, 0, 2] != sym[0, 1, 2]
    assert dists[0] == [[0, 0, 1], [0, 0, 1], [1, 1, 0]] and picks == [0, None, 0] and risks[0] == [1 / 17, 1 / 17, 2 / 17]
    # the example of INTEGRATION.md: under unit costs the reading with the real error is picked and its error is voted through, in a
    # network with a column too many; under historic_latin() the error is voted away
    unit = s2s.confusion_of([READINGS])
    costed = s2s.confusion_of([READINGS], costs=hl)
    assert s2s.consensus_of([READINGS])[0] == [2] and unit[2] == [2] and costed[2] == [0]
    assert unit[0] == ['Waſſer is selten'] and costed[0] == ['Waſſer ist selten']
    assert len(unit[1][0]) == 18 and len(costed[1][0]) == 17
    assert costed[3][0][2] == [('ſ', 2.0, [0, 2]), ('s', 1.0, [1])]                    # keys never pool votes: two classes of one column
    assert [c[0] for c in s2s.engine.calls if isinstance(c[0], str)][-3:] == ['costed', 'align_costed', 'vote']
    # correct_candidates and consensus_lines hand their costs on
    seen = {}
    s2s.confusion_of = lambda *a, **kw: seen.update(kw) or ([''], [[]], [None], [[]])
    s2s.correct_candidates([READINGS], costs=hl)
    assert seen['costs'] is hl
    s2s.correct_candidates([READINGS])
    assert 'costs' not in seen or seen.pop('costs') is hl


def test_the_facade_refuses():
    from cor_asv_ann_amd.edit_costs import EditCosts
    s2s = _stub_facade(8)
    graded = EditCosts.graded()
    for call in (s2s.consensus_of, s2s.confusion_of):
        call([['a' * 2048, 'b']], costs=graded)
        with pytest.raises(ValueError):
            call([['a' * 2049, 'b']], costs=graded)
    s2s.consensus_of([['a' * 2049, 'b']])                        # (the plain vote takes 8192)
    assert [c[0] for c in s2s.engine.calls if isinstance(c[0], str)] == ['costed', 'costed', 'align_costed', 'vote']


class _Proposal(object):
    """sample_lines answered from a list, consensus_of by the facade on the stub engine."""

    def __init__(self, drawn):
        self.s2s, self.drawn = _stub_facade(64), drawn

    def sample_lines(self, src, conf, n, **kw):
        return ([list(d[:n]) for d in self.drawn],)

    def consensus_of(self, *a, **kw):
        return self.s2s.consensus_of(*a, **kw)


def test_risk_candidates_cost_under_the_costs():
    from cor_asv_ann_amd.edit_costs import EditCosts
    from cor_asv_ann_amd.training import risk_candidates
    gold = ['Waſſer iſt ſelten', 'abc']
    drawn = [['Wasser ist selten', 'Waſſer iſt ſelten', 'Waſſer is selten'], ['Abc', 'abd', 'ab']]
    settings = dict(samples=4, temperature=1.0, top_k=0, top_p=1.0, seed=1)
    cands, cost = risk_candidates(_Proposal(drawn), ['x', 'y'], None, gold, settings, 0)
    assert cands == [[g] + d for g, d in zip(gold, drawn)]
    assert cost.dtype == np.float32 and np.array_equal(cost, np.array([0, 4 / 17, -1, 3 / 17, 0, 1 / 3, 1 / 3, 1 / 3], np.float32))
    # historic_latin(): the sample with s for ſ costs 0 and is no duplicate of the gold line; the exact copy still is one
    _, cost = risk_candidates(_Proposal(drawn), ['x', 'y'], None, gold, dict(settings, edit_costs=EditCosts.historic_latin()), 0)
    assert np.array_equal(cost, np.array([0, 0, -1, 1 / 17, 0, 1 / 3, 1 / 3, 1 / 3], np.float32))
    # graded(): case and long s cost half an edit -- 1 over unit 2 x the characters; a deletion a whole one
    _, cost = risk_candidates(_Proposal(drawn), ['x', 'y'], None, gold, dict(settings, edit_costs=EditCosts.graded()), 0)
    assert np.array_equal(cost[4:], np.array([0, 1 / 6, 2 / 6, 2 / 6], np.float32)) and cost[1] == cost[3] == np.float32(4 / 34)


def test_train_records_only_what_it_can_name():
    from cor_asv_ann_amd.edit_costs import EditCosts
    from cor_asv_ann_amd.training import check_risk_resume, train_files
    assert EditCosts.historic_latin().settings() == {'gap': 1, 'sub': 1, 'near': 0, 'unit': 1, 'key': 'historic_latin'}
    assert EditCosts(2, 3, 1).settings() == {'gap': 2, 'sub': 3, 'near': 1, 'unit': 3, 'key': None}
    with pytest.raises(ValueError):
        EditCosts(2, 2, 1, key=str.lower).settings()
    s2s = _stub_facade(8)
    with pytest.raises(ValueError):
        train_files(s2s, [], risk_costs=EditCosts.graded())                              # without risk_samples
    # resume refuses a mismatch in either direction; without costs on both sides nothing is compared
    base = dict(samples=4, alpha=1.0, temperature=1.0, top_k=0, top_p=1.0, own_proposal=True)
    graded, hl = EditCosts.graded().settings(), EditCosts.historic_latin().settings()
    check_risk_resume({'risk': dict(base, seed=3)}, 'f', dict(base))
    check_risk_resume({'risk': dict(base, seed=3, costs=graded)}, 'f', dict(base, costs=EditCosts.graded().settings()))
    for theirs, mine in ((dict(base), dict(base, costs=graded)), (dict(base, costs=graded), dict(base)), (dict(base, costs=graded), dict(base, costs=hl))):
        with pytest.raises(ValueError):
            check_risk_resume({'risk': theirs}, 'f', mine)


def test_the_entries_are_bound():
    from ctypes import POINTER, c_int, c_int32, c_void_p, sizeof
    from cor_asv_ann_amd import _native as nv
    assert sizeof(nv.EditCosts) == 16 and [f[0] for f in nv.EditCosts._fields_] == ['gap', 'sub', 'near', 'unit']
    assert nv.SIGNATURES['casv_consensus_costed'] == (c_int, [c_void_p] + [c_int32] * 4 + [c_void_p] * 4 + [POINTER(nv.EditCosts)] + [c_void_p] * 3)
    assert nv.SIGNATURES['casv_consensus_align_costed'] == (c_int, [c_void_p] + [c_int32] * 3 + [c_void_p] * 4 + [POINTER(nv.EditCosts)] + [c_void_p] * 2)
