"""Weighted edit costs on the device (csrc/consensus_kernels.hip: consensus_dist_costed_kernel, consensus_align_costed_kernel;
csrc/consensus.hip: casv_consensus_costed; csrc/consensus_align.hip: casv_consensus_align_costed) against
the restatement of tests/cost_cases.py, which tests/test_cost_cases.py holds on the CPU -- with the condition that every wrong
variant differs from it on a case run here.  Everything is compared for exact equality: int32 distances, picks, where, ncol, src
and best, float64 risks and masses bit for bit.  Runs with and without CASV_POISON=1."""
import os
from ctypes import byref, c_int64

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

os.environ.setdefault('CASV_POISON', '1')      # read once by the library, at its first allocation

from tests import align_cases as ac
from tests import consensus_cases as cc
from tests import cost_cases as k
from tests import sample_cases as sa

ERR_ARG = -1


@pytest.fixture(scope='module')
def eng():
    """A handle without weights: the costed calls need none."""
    from cor_asv_ann_amd.engine import HipEngine
    e = HipEngine(1, 32, 12)
    yield e
    e.close()


def _run(eng, sym, key, length, pivot, w, mode, costs, C=None):
    """(risk, pick, dist, where, ncol, src, mass, best): both costed calls and one vote."""
    risk, pick, dist = eng.consensus(sym, length, weights=w, mode=mode, want_dist=True, key=key, costs=costs)
    where, ncol = eng.consensus_align(sym, length, pivot, key=key, costs=costs)
    return (risk, pick, dist, where, ncol) + eng.consensus_vote(max(1, int(ncol.max())) if C is None else C, weights=w)


def _plain(eng, sym, length, pivot, w, mode):
    risk, pick, dist = eng.consensus(sym, length, weights=w, mode=mode, want_dist=True)
    where, ncol = eng.consensus_align(sym, length, pivot)
    return (risk, pick, dist, where, ncol) + eng.consensus_vote(max(1, int(ncol.max())), weights=w)


def _stat(eng, key):
    value = c_int64(0)
    assert eng.lib.casv_get_stat(eng.handle, key.encode(), byref(value)) == 0
    return value.value


# ------------------------------------------------------------------------------------------------------------------ a. the cases
@pytest.mark.parametrize('name', k.CASE_IDS)
def test_case_against_the_restatement(eng, name):
    """Lengths 0 .. 200 against each other per alphabet and cost set, 2048 x 2048 at costs of 255, 3 x 65 both ways, N = 1 .. 256
    with padding, 66000 sources, odd symbols and keys, no keys, keys per position, weights in both modes."""
    got = _run(eng, *k.case(name))
    want = k.expected(name)
    for what, g, w in zip(('risk', 'pick', 'dist', 'where', 'ncol', 'src', 'mass', 'best'), got, want):
        assert k.same((g,), (w,)), what


@pytest.mark.parametrize('name', ('lengths_four_1_1_1_u1', 'lengths_two_2_3_1_u3', 'shape_N65_B2', 'weights_mode1', 'odd_symbols_and_keys'))
def test_unit_costs_without_keys_are_the_plain_calls(eng, name):
    sym, _, length, pivot, w, mode, _ = k.case(name)
    plain = _plain(eng, sym, length, pivot, w, mode)
    assert k.same(_run(eng, sym, None, length, pivot, w, mode, k.UNIT), plain)
    assert k.same(plain[:3], cc.reference(sym, length, w, mode)) and k.same(plain[3:], ac.reference(sym, length, pivot, w))


@pytest.mark.parametrize('name', ('lengths_four_2_3_1_u3', 'lengths_three_1_1_0_u1', 'weights_mode1', 'shape_N64_B2', 'odd_symbols_and_keys'))
def test_symbols_and_keys_beyond_a_length_influence_nothing(eng, name):
    sym, key, length, pivot, w, mode, costs = k.case(name)
    p_sym, p_key = k.poisoned(sym, key, length, seed=3)
    assert k.same(_run(eng, p_sym, p_key, length, pivot, w, mode, costs), k.expected(name))
    noise = np.random.default_rng(4).integers(cc.I32_MIN, cc.I32_MAX, sym.shape, dtype=np.int64, endpoint=True).astype(np.int32)
    beyond = np.arange(sym.shape[2])[None, None, :] >= np.maximum(length, 0)[:, :, None]
    assert k.same(_run(eng, np.where(beyond, noise, sym), np.where(beyond, noise[::-1], key), length, pivot, w, mode, costs), k.expected(name))


def test_a_wider_L_changes_nothing(eng):
    """The same candidates in a call of L = 2048: the LDS of a wave follows the longest live candidate, not L."""
    sym, key, length, pivot, w, mode, costs = k.case('weights_mode1')
    wide, wide_key = np.full(sym.shape[:2] + (k.MAX_L,), 7, np.int32), np.full(sym.shape[:2] + (k.MAX_L,), 1, np.int32)
    wide[:, :, :sym.shape[2]], wide_key[:, :, :sym.shape[2]] = sym, key
    got = _run(eng, wide, wide_key, length, pivot, w, mode, costs)
    want = k.expected('weights_mode1')
    assert np.array_equal(got[3][:, :, :sym.shape[2]], want[3]) and (got[3][:, :, sym.shape[2]:] == ac.NONE).all()
    assert k.same(got[:3] + got[4:], want[:3] + want[4:])


# ------------------------------------------------------------------------------------------------------------------ b. independence
def test_sources_are_independent_of_each_other_and_of_B(eng):
    name = 'weights_mode1'
    sym, key, length, pivot, w, mode, costs = k.case(name)
    want = k.expected(name)
    B = sym.shape[0]
    perm = np.random.default_rng(0).permutation(B)
    assert k.same(_run(eng, sym[perm], key[perm], length[perm], pivot[perm], w[perm], mode, costs, C=want[5].shape[1]), tuple(x[perm] for x in want))
    for b in range(B):                                                              # a source alone
        one = slice(b, b + 1)
        got = _run(eng, sym[one], key[one], length[one], pivot[one], w[one], mode, costs, C=want[5].shape[1])
        assert k.same(got, tuple(x[one] for x in want))
    rep = np.arange(B).repeat(40)                                                   # and among 160
    got = _run(eng, sym[rep], key[rep], length[rep], pivot[rep], w[rep], mode, costs)
    assert k.same(got, tuple(x[rep] for x in want))


@pytest.mark.parametrize('name,budget,rounds', [('weights_mode0', 1, 4), ('lengths_four_2_2_1_u2', 4 * 13 * 200 * 7 * 8, 4)])
def test_rounds_under_a_small_budget_change_nothing(eng, name, budget, rounds):
    case = k.case(name)
    assert k.same(_run(eng, *case), k.expected(name)) and _stat(eng, 'align_rounds') == 1
    eng.debug_set_align_budget(budget)
    try:
        got = _run(eng, *case)
        assert _stat(eng, 'align_rounds') == rounds >= 3
    finally:
        eng.debug_set_align_budget(0)
    assert k.same(got, k.expected(name))


def test_plain_and_costed_calls_give_their_own_results_in_any_order(eng):
    """A plain call after a costed one and a costed one after a plain one, distances and alignments; a vote reads the last align,
    costed or not."""
    name = 'lengths_four_2_3_1_u3'
    sym, key, length, pivot, w, mode, costs = k.case(name)
    want = k.expected(name)
    plain = cc.reference(sym, length, w, mode), ac.Reference()
    plain_align = plain[1].align(sym, length, pivot)
    assert not np.array_equal(plain_align[0], want[3]) and not np.array_equal(plain[0][2], want[2])       # (the case tells them apart)
    C = max(int(want[4].max()), int(plain_align[1].max()))
    costed_ref = k.Reference(costs)
    costed_ref.align(sym, length, pivot, key)
    for _ in range(2):
        assert k.same(eng.consensus(sym, length, weights=w, mode=mode, want_dist=True, key=key, costs=costs), want[:3])
        assert k.same(eng.consensus(sym, length, weights=w, mode=mode, want_dist=True), plain[0])
        assert k.same(eng.consensus_align(sym, length, pivot, key=key, costs=costs), want[3:5])
        assert k.same(eng.consensus_vote(C), costed_ref.vote(C))                     # the costed alignment
        assert k.same(eng.consensus(sym, length, weights=w, mode=mode, want_dist=True), plain[0])
        assert k.same(eng.consensus_vote(C), costed_ref.vote(C))                     # ... still, behind a plain distance call
        assert k.same(eng.consensus_align(sym, length, pivot), plain_align)
        assert k.same(eng.consensus_vote(C), plain[1].vote(C))


# ------------------------------------------------------------------------------------------------------------------ c. refusals
def _raw(eng, what, B, N, L, mode, sym, key, length, w, pivot, costs, outs):
    from cor_asv_ann_amd import _native as nv
    c = None if costs is None else byref(nv.EditCosts(*costs))
    if what == 'dist':
        return eng.lib.casv_consensus_costed(eng.handle, B, N, L, mode, nv.ptr(sym), nv.ptr(key), nv.ptr(length), nv.ptr(w), c,
                                             nv.ptr(outs[0]), nv.ptr(outs[1]), nv.ptr(outs[2]))
    return eng.lib.casv_consensus_align_costed(eng.handle, B, N, L, nv.ptr(sym), nv.ptr(key), nv.ptr(length), nv.ptr(pivot), c,
                                               nv.ptr(outs[0]), nv.ptr(outs[1]))


def _refusals(eng):
    """After a served costed align: every refused argument answers CASV_ERR_ARG and writes nothing, and a vote afterwards still
    reads the served align."""
    name = 'weights_mode0'
    case = k.case(name)
    want = k.expected(name)
    assert k.same(_run(eng, *case), want)
    kept_C = want[5].shape[1]
    B, N, L = 2, 3, 4
    sym, key = np.ones((B, N, L), np.int32), np.zeros((B, N, L), np.int32)
    length, pivot = np.array([[2, 2, -1], [2, 0, 4]], np.int32), np.array([1, -1], np.int32)
    ok = dict(B=B, N=N, L=L, mode=0, sym=sym, key=key, length=length, w=None, pivot=pivot, costs=(2, 3, 1, 3))
    bad_costs = [None, (0, 1, 1, 1), (256, 1, 1, 1), (-1, 1, 1, 1), (1, 256, 1, 1), (1, 2, 3, 1), (1, 1, -1, 1), (1, -1, -1, 1), (1, 1, 1, 0),
                 (1, 1, 1, 256), (1, 300, 300, 1)]
    bad = [dict(costs=c) for c in bad_costs] + [dict(L=2049), dict(L=-1), dict(B=0), dict(N=0), dict(N=257), dict(sym=None), dict(length=None),
                                                dict(length=np.array([[2, 2, -2], [2, 2, 2]], np.int32)), dict(length=np.array([[2, 2, 2], [2, 5, 2]], np.int32))]
    w = np.ones((B, N))
    w[1, 2] = np.nan
    for what, more in (('dist', [dict(mode=2), dict(mode=-1), dict(w=w)]),
                       ('align', [dict(pivot=None), dict(pivot=np.array([3, 0], np.int32)), dict(pivot=np.array([2, 0], np.int32))])):
        for change in bad + more:
            outs = (np.full((B, N, N), 77, np.int32), np.full((B, N), 77.0), np.full((B,), 77, np.int32)) if what == 'dist' else \
                (np.full((B, N, L), 77, np.int32), np.full((B,), 77, np.int32))
            assert _raw(eng, what, outs=outs, **dict(ok, **change)) == ERR_ARG, (what, change)
            assert all((o == 77).all() for o in outs), (what, change)
        assert b'' != eng.lib.casv_last_error()
    # the served align is still there, whole
    assert k.same(eng.consensus_vote(kept_C, weights=case[4]), want[5:])
    # what is allowed: no keys; L = 0 without symbols, keys or where; the largest costs
    outs = np.full((B, N, N), 77, np.int32), np.full((B, N), 77.0), np.full((B,), 77, np.int32)
    assert _raw(eng, 'dist', outs=outs, **dict(ok, key=None, costs=(255, 255, 255, 255))) == 0
    assert outs[0].tolist() == [[[0, 0, -1], [0, 0, -1], [-1, -1, -1]], [[0, 510, 510], [510, 0, 1020], [510, 1020, 0]]]
    zero = np.zeros((B, N), np.int32)
    assert _raw(eng, 'dist', outs=outs, **dict(ok, L=0, sym=None, key=None, length=zero)) == 0 and (outs[0] == 0).all()
    ncol = np.full((B,), 77, np.int32)
    assert _raw(eng, 'align', outs=(None, ncol), **dict(ok, L=0, sym=None, key=None, length=zero, pivot=np.array([0, 2], np.int32))) == 0
    assert ncol.tolist() == [0, 0]


def test_refused_arguments(eng):
    _refusals(eng)


def test_other_entry_points_are_untouched_by_the_costed_calls():
    """A sampling call, a greedy decode and a scoring call give the same bits with costed calls (served or refused) before, between
    and behind them as without; the costed calls run before any weights exist."""
    from cor_asv_ann_amd.engine import HipEngine
    case = sa.BATCH_CASE
    mc = sa.build_model(case)
    model = HipEngine(case[1], case[2], case[3], **mc['flags'])
    name = 'weights_mode1'
    try:
        assert k.same(_run(model, *k.case(name)), k.expected(name))                   # before any weights are committed
        model.set_weights(mc['w'])
        idx = mc['idx']
        din = np.where(idx >= 0, np.roll(idx, 1, axis=1), -1).astype(np.int32)
        din[:, 0] = -1

        def others(costed):
            costed()
            model.encode(idx)
            costed()
            s = model.decode_sample(3, seed=1, temperature=0.9, top_k=5, want_align=True)
            costed()
            g = model.decode_greedy(mode=0, want_align=True)
            costed()
            t = model.score_targets(idx, None, din, idx)[:5]
            costed()
            return list(s) + list(g) + list(t)

        def costed():
            assert k.same(_run(model, *k.case(name)), k.expected(name))

        before = others(lambda: None)
        for between in (costed, lambda: _refusals(model)):
            after = others(between)
            for x, y in zip(before, after):
                assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()
    finally:
        model.close()


def test_the_costed_calls_are_timed_under_the_vote_s_class(eng):
    sym, key, length, pivot, w, mode, costs = k.case('asymmetric_3_65')
    eng.profile(True)
    before = eng.profile_read('consensus')['launches']
    eng.consensus(sym, length, key=key, costs=costs)
    eng.consensus_align(sym, length, pivot, key=key, costs=costs)
    after = eng.profile_read('consensus')
    assert after['launches'] == before + 2 and after['ms'] > 0
    eng.profile(False)


# ------------------------------------------------------------------------------------------------------------------ d. end to end
READINGS = ['Waſſer iſt ſelten', 'Wasser ist selten', 'Waſſer is selten']       # INTEGRATION.md's example (tests/test_cost_cases.py)


def test_consensus_of_and_confusion_of_end_to_end():
    """Three engines' readings of a Fraktur line on an unconfigured facade: under unit costs the reading with the real error is
    picked and the error is voted through; under historic_latin() it is voted away.  Each equal to the restatement's answer."""
    from cor_asv_ann_amd.edit_costs import EditCosts
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence
    s2s, stub = Sequence2Sequence(), Sequence2Sequence()
    stub.engine = k.StubEngine()
    cands = [READINGS, [], ['Straße', 'strasse', 'Strafse', 'STRASSE']]
    try:
        for costs in (None, EditCosts.historic_latin(), EditCosts.graded(), EditCosts(2, 3, 1, key={ord('ß'): 1, ord('s'): 1})):
            kw = {} if costs is None else {'costs': costs}
            for normalise in (False, True):
                assert s2s.consensus_of(cands, normalise=normalise, distances=True, **kw) == stub.consensus_of(cands, normalise=normalise, distances=True, **kw)
            assert s2s.confusion_of(cands, weights=[[1.0, 1.0, 1.5], None, None], **kw) == stub.confusion_of(cands, weights=[[1.0, 1.0, 1.5], None, None], **kw)
        hl = EditCosts.historic_latin()
        assert s2s.consensus_of([READINGS])[0] == [2] and s2s.consensus_of([READINGS], costs=hl)[0] == [0]
        unit, costed = s2s.confusion_of([READINGS]), s2s.confusion_of([READINGS], costs=hl)
        assert unit[0] == ['Waſſer is selten'] and costed[0] == ['Waſſer ist selten']
        assert len(unit[1][0]) == 18 and len(costed[1][0]) == 17 and costed[3][0][2] == [('ſ', 2.0, [0, 2]), ('s', 1.0, [1])]
        assert s2s.consensus_of([READINGS], costs=hl, distances=True)[2] == [[[0, 0, 1], [0, 0, 1], [1, 1, 0]]]
    finally:
        s2s._vote_engine.close()
