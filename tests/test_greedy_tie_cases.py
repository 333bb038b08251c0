"""The greedy tie cases (tests/greedy_tie_cases.py), checked on the CPU: what tests/test_gpu_greedy_ties.py compares the device with
is decided by the pick rules and not by rounding, is really made of ties, exact ones and zeros, reaches all four forms of the pick,
and would change if a rule did."""
import os

import numpy as np
import pytest

from oracle.decode import decode_batch_greedy, decode_sequence_greedy
from tests.greedy_tie_cases import CASES, BY_NAME, MODES, RULES, NEGATIVE_ROWS, greedy_form, pick, run

_runs = {}
NAMES = [c.name for c in CASES]
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'cor_asv_ann_amd', 'csrc')


def _run(case, mode, dtype=np.float32, rules=(), nan_row='case'):
    key = (case.name, mode, np.dtype(dtype).name, tuple(rules), nan_row)
    if key not in _runs:
        _runs[key] = run(case, mode, dtype, rules, nan_row)
    return _runs[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _decisions(res):
    """What two decodes of a case must share: every reported index, the lengths, the raises."""
    return [(tuple(res['idx'][j, :res['length'][j]]), int(res['length'][j]), bool(res['raised'][j])) for j in range(len(res['length']))]


def _first_step(case, dtype=np.float32):
    m = case.model(dtype)
    enc = case.encoder_outputs(m)
    p, _ = m.step(np.zeros((case.B, case.V), np.uint32), enc[0], list(enc[1:]))
    return p


def _rows(case):
    """-> (rows of positive h, rows of negative h); the NaN row is in neither."""
    neg = [r for r in NEGATIVE_ROWS if r < case.B] if case.explicit else []
    return [r for r in range(case.B) if r not in neg and r != case.nan_row], neg


@pytest.mark.parametrize('name', NAMES)
def test_the_restated_loop_with_no_switch_is_the_oracle(name):
    """Mode 0 against decode_batch_greedy (every step of every row: indices, probabilities bit for bit, the alignments of a line's
    reported part) where the case starts from the encoder; mode 1 against decode_sequence_greedy line by line, handed the case's
    encoder outputs: characters, probabilities and alignments bit for bit, and a raise exactly where the restatement has one."""
    case = BY_NAME[name]
    m = case.model()
    enc = case.encoder_outputs(m)
    c_i = m.mapping[0]
    if not case.explicit:
        got = _run(case, 0)
        want = decode_batch_greedy(m, case.inputs(m)[0], return_indexes='probs')
        assert np.array_equal(got['idx'], want[5])
        assert np.array_equal(_bits(got['prob']), _bits(want[6]))
        for j in range(case.B):
            a = np.asarray(want[4][j])
            assert np.array_equal(got['align'][j, :len(a)], a)
    got = _run(case, 1)
    for j in range(case.B):
        n = int(got['length'][j])
        try:
            with np.errstate(divide='ignore'):          # (-log of a saturated row's 0.0)
                text, probs, _, aligns = decode_sequence_greedy(m, encoder_outputs=[e[j:j + 1] for e in enc])
        except ValueError:
            assert got['raised'][j] and got['idx'][j, n - 1] == 1 and np.isnan(got['prob'][j, n - 1]), j
            continue
        assert not got['raised'][j], j
        assert [c_i[ch] for ch in text] == list(got['idx'][j, :n]), j
        assert np.array_equal(_bits(got['prob'][j, :n]), _bits(probs)), j
        assert np.array_equal(got['align'][j, :n], np.asarray(aligns)), j


@pytest.mark.parametrize('name', [c.name for c in CASES if not c.saturated])
def test_the_fp32_and_the_fp64_oracle_agree(name):
    """No exclusions: every index, length and raise of every line, in both modes.  The fp64 side: decode_batch_greedy (the
    restatement where the case hands in encoder outputs) and decode_sequence_greedy per line."""
    case = BY_NAME[name]
    m = case.model(np.float64)
    enc = case.encoder_outputs(m)
    c_i = m.mapping[0]
    got = _run(case, 0)
    if case.explicit:
        assert np.array_equal(got['idx'], _run(case, 0, np.float64)['idx'])
    else:
        assert np.array_equal(got['idx'], decode_batch_greedy(m, case.inputs(m)[0], return_indexes=True)[5])
    got = _run(case, 1)
    for j in range(case.B):
        n = int(got['length'][j])
        try:
            text = decode_sequence_greedy(m, encoder_outputs=[e[j:j + 1] for e in enc])[0]
        except ValueError:
            assert got['raised'][j], j
            # (up to the raise the restatement in fp64 says what the reference had picked)
            assert _decisions(_run(case, 1, np.float64))[j] == _decisions(got)[j]
            continue
        assert not got['raised'][j] and [c_i[ch] for ch in text] == list(got['idx'][j, :n]), j


@pytest.mark.parametrize('name', NAMES)
def test_the_ties_are_exact_and_the_promises_hold(name):
    """In the fp32 oracle the probabilities at a case's tied indices are bitwise equal and strictly above every other entry; a
    strict pair is at least 1e-3 apart in fp64, relative -- 5x the 2e-4 the device's probabilities are held to, so rounding
    there cannot turn the order; the table's promises about picks, lengths and raises hold."""
    case = BY_NAME[name]
    pr = case.promises
    p = _first_step(case)
    pos, neg = _rows(case)
    assert pos and (not case.explicit or neg)
    for rows, key in ((pos, 'tie'), (neg, 'neg')):
        tie = list(pr.get(key, ()))
        others = [v for v in range(case.V) if v not in tie]
        for r in rows:
            if tie:
                assert len(set(_bits(p[r, tie]).tolist())) == 1, (r, key)
                assert not others or p[r, tie[0]] > p[r, others].max(), (r, key)
    if 'strict' in pr:
        hi, lo = pr['strict']
        p64 = _first_step(case, np.float64)
        for r in pos:
            assert p[r, hi] > p[r, lo] > np.delete(p[r], [hi, lo]).max()
            assert (p64[r, hi] - p64[r, lo]) / p64[r, hi] >= 1e-3
    if case.family == 'uniform':
        assert np.array_equal(_bits(p), _bits(np.full(p.shape, np.float32(1) / np.float32(case.V))))
    else:
        n = len({int(b) for b in _bits(p[pos, 5])})
        assert n > len(pos) // 2 if case.explicit else n == 1      # rows differ only where states do
    r0, r1 = _run(case, 0), _run(case, 1)
    if case.family == 'uniform':                       # fl32(1/V) at every step; mode 1 ends every line with its first pick
        assert (_bits(r0['prob']) == _bits(np.float32(1) / np.float32(case.V))).all() and (r1['length'] == 1).all()
    for r in pos:
        assert (r0['idx'][r] == pr['pick0']).all() and not r0['all_nan'][r].any(), r
        assert r1['idx'][r, 0] == pr['pick1'] and r1['raised'][r] == pr['err1'], r
        assert r1['length'][r] == (pr['len1'] or case.S), r
        assert r1['nan0'][r, 0] == (0 in pr.get('tie', ()) or pr.get('strict', (1,))[0] == 0 or (case.saturated and case.sets[0] == (0,))), r
        assert not r0['nan0'][r].any() and np.isfinite(r0['prob'][r]).all(), r          # mode 0 feeds nothing back but the distribution
    for r in neg:
        assert (r0['idx'][r] == min(pr['neg'])).all() and r1['idx'][r, 0] == min(pr['neg']), r
    if case.explicit:
        assert {int(r1['length'][r]) for r in neg} == ({1} if min(pr['neg']) == 1 else {case.S})


@pytest.mark.parametrize('name', [c.name for c in CASES if c.saturated])
def test_saturated_rows_are_exact_in_any_float32_exp(name):
    """The zeros of a saturated row lie at least 150 below the top logit in fp64 (float32's smallest denormal is exp(-103.3)), so
    they are 0 whatever the exp; the denormal entry lies in [-100, -90], inside the denormal range (exp(-87.3) is the smallest
    normal) with margin on both sides.  The fp32 oracle has exactly 1.0, 0.0 and one denormal, and picks the denormal in mode 0."""
    case = BY_NAME[name]
    top = case.sets[0][0]
    d = case.promises.get('denormal')
    with np.errstate(divide='ignore'):
        gap = np.log(_first_step(case, np.float64))
    gap -= gap[:, top:top + 1]
    zeros = [v for v in range(case.V) if v not in (top, d)]
    assert gap[:, zeros].max() <= -150
    p = _first_step(case)
    assert (p[:, top] == 1).all() and not p[:, zeros].any()
    if d is not None:
        assert (-100 <= gap[:, d]).all() and (gap[:, d] <= -90).all()
        assert (p[:, d] > 0).all() and (p[:, d] < np.finfo(np.float32).tiny).all()
        assert (_run(case, 0)['idx'] == d).all()
    for mode in MODES:
        res = _run(case, mode)
        for j in range(case.B):
            n = int(res['length'][j]) - int(res['raised'][j])
            assert all(x in (0.0, 1.0) or (d is not None and k == d) for k, x in zip(res['idx'][j, :n], res['prob'][j, :n]))


@pytest.mark.parametrize('name', [c.name for c in CASES if c.nan_row is not None])
def test_the_nan_row_is_alone(name):
    """Mode 0: the row reports index 1 and NaN at every step, every other row keeps the bits it has with that row finite.  Mode 1:
    the row raises with length 1, the others' reported parts are unchanged."""
    case = BY_NAME[name]
    r = case.nan_row
    assert 0 < r < case.B - 1 and (case.B < 16 or (r % 4 not in (0, 3) and r % 16 not in (0, 15)))
    for mode in MODES:
        got, clean = _run(case, mode), _run(case, mode, nan_row=None)
        assert got['all_nan'][r, 0] and got['idx'][r, 0] == 1 and np.isnan(got['prob'][r, 0])
        if mode == 0:
            assert got['all_nan'][r].all() and (got['idx'][r] == 1).all() and np.isnan(got['prob'][r]).all()
        else:
            assert got['raised'][r] and got['length'][r] == 1
        others = [j for j in range(case.B) if j != r]
        assert not got['all_nan'][others].any() and not got['raised'][others].any()
        for key in ('idx', 'length', 'raised'):
            assert np.array_equal(got[key][others], clean[key][others]), key
        assert np.array_equal(_bits(got['prob'][others]), _bits(clean['prob'][others]))
        assert np.array_equal(_bits(got['align'][others]), _bits(clean['align'][others]))


# rule -> (case, mode) it must flip, and why
FLIPS = {
    'tie_high': ('q_v40_5_21', 0, 'the tie (5, 21) goes to 21'),
    'zero_in_mode0': ('z_v40_above', 0, 'index 0, on top, is picked'),
    'zero_gt': ('z_v40_tie7', 1, 'index 0 only ties 7: no NaN, the line runs its 2T steps without a raise'),
    'no_writeback': ('z_v40_tie7', 1, 'the NaN is not fed back: the next step is finite, no raise'),
    'writeback_mode0': ('z_v40_tie7', 0, 'the NaN is fed back in mode 0: every later step reports index 1 and NaN'),
}


@pytest.mark.parametrize('rule', RULES)
def test_a_flipped_rule_changes_an_expected_output(rule):
    """The comparison can fail: with one switch set the restated loop returns something else on the case named for it."""
    name, mode, why = FLIPS[rule]
    changed = [(c.name, mode_) for c in CASES for mode_ in MODES
               if _decisions(_run(c, mode_, rules=(rule,))) != _decisions(_run(c, mode_))]
    print('%s changes %d of %d decodes: %s' % (rule, len(changed), 2 * len(CASES), changed))
    assert (name, mode) in changed, why
    base, flipped = _run(BY_NAME[name], mode), _run(BY_NAME[name], mode, rules=(rule,))
    if rule == 'tie_high':
        assert (base['idx'] == 5).all() and (flipped['idx'] == 21).all()
    elif rule == 'zero_in_mode0':
        assert (base['idx'] == 7).all() and (flipped['idx'] == 0).all()
    elif rule in ('zero_gt', 'no_writeback'):
        assert base['raised'].all() and (base['length'] == 2).all()
        assert not flipped['raised'].any() and (flipped['length'] == BY_NAME[name].S).all() and (flipped['idx'] == 7).all()
    else:
        assert (base['idx'] == 7).all() and (flipped['idx'][:, 0] == 7).all()
        assert (flipped['idx'][:, 1:] == 1).all() and np.isnan(flipped['prob'][:, 1:]).all()
    # a switch that does nothing where its rule does not bear: mode 0 ignores the three mode-1 switches and the other way round
    other = {'zero_in_mode0': 1, 'writeback_mode0': 1, 'zero_gt': 0, 'no_writeback': 0}.get(rule)
    if other is not None:
        assert all(_decisions(_run(c, other, rules=(rule,))) == _decisions(_run(c, other)) for c in CASES if c.V <= 40)


def test_pick_on_rows_written_by_hand():
    nan = np.float32(np.nan)
    f = lambda *x: np.array(x, np.float32)
    assert pick(f(.1, .2, .3, .3), 0)[:1] == (2,) and pick(f(.1, .2, .3, .3), 0, ('tie_high',))[0] == 3
    assert pick(f(.5, .2, .3), 0) == (2, np.float32(.3), False, False) and pick(f(.5, .2, .3), 1) == (2, np.float32(.3), True, False)
    assert pick(f(.3, .2, .3), 1)[2] and not pick(f(.3, .2, .3), 1, ('zero_gt',))[2] and not pick(f(.3, .2, .3), 1, ('no_writeback',))[2]
    assert pick(f(.5, .2, .3), 0, ('zero_in_mode0',))[0] == 0 and pick(f(.5, .2, .3), 0, ('writeback_mode0',))[2]
    assert pick(f(nan, .2, .3), 1) == (2, np.float32(.3), False, False)                  # `p0 == p0`
    assert pick(f(.1, nan, .3, nan), 0)[0] == 2                                          # nanargmax skips NaN
    for mode in MODES:
        k, p, nan0, all_nan = pick(f(.4, nan, nan), mode)                                # a finite p[0] does not save the row
        assert (k, nan0, all_nan) == (1, False, True) and np.isnan(p)


def test_the_table_reaches_all_four_forms():
    """greedy_form restates the dispatch of persist_decode_kernel; its premise -- Vp = (V + 31) & ~31 -- and the dispatch itself are
    read back from the sources."""
    with open(os.path.join(CSRC, 'engine.hip')) as f:
        assert 'm->Vp = (cfg->voc_size + 31) & ~31;' in f.read()
    with open(os.path.join(CSRC, 'persist.hip')) as f:
        src = f.read()
    assert 'if (V == 256 && Vp == 256) row_stats_quarter<true>(' in src and 'else if (V <= 256) row_stats_quarter<false>(' in src
    assert [greedy_form(V) for V in (2, 40, 224, 255, 256, 257, 640)] == ['quarter'] * 4 + ['quarter_full', 'wave', 'wave']
    for form in ('quarter', 'quarter_full', 'wave'):            # (the per-step kernel runs every case)
        sel = [c for c in CASES if c.form == form]
        assert {c.family for c in sel} == {'uniform', 'tied'}
        assert any(c.explicit and c.nan_row is None for c in sel) and any(c.nan_row is not None for c in sel)
        assert any(c.saturated for c in sel) and any('denormal' in c.promises for c in sel)
        assert any(0 in c.promises.get('tie', ()) and c.family == 'tied' for c in sel) and any('strict' in c.promises for c in sel)
        assert {c.B for c in sel} >= {3, 37} or form == 'quarter_full'
        assert any(c.B > 16 for c in sel)
    assert {c.B for c in CASES} == {1, 3, 17, 37} and {c.V for c in CASES} == {2, 12, 40, 255, 256, 257, 640}
    assert all(c.T <= 5 and 1 <= min(map(len, c.lines)) and max(map(len, c.lines)) <= 4 for c in CASES)
    assert all(len(set(map(len, c.lines))) > 1 for c in CASES if c.B > 1)                # ragged
    assert all(c.B % 16 for c in CASES)                                                  # the last row block is partial: rq < R clamps
    # the lane structure: same lane / other slot, each butterfly partner of the quarter, lane 0 past index 0, passes of the whole wave
    quarter = {c.sets[0] for c in CASES if c.form != 'wave' and c.family == 'tied' and not c.explicit}
    assert quarter >= {(5, 21), (21, 37), (5, 13), (5, 9), (5, 7), (5, 4), (9, 13), (16, 32, 1), (13, 5, 9)}
    assert {a ^ b for a, b in (s for s in quarter if len(s) == 2 and max(s) < 16)} >= {8, 4, 2, 1}          # lane_xor<8>, <4>, <2>, <1>
    wave = {c.sets[0] for c in CASES if c.form == 'wave' and c.family == 'tied' and not c.explicit}
    assert wave >= {(5, 69), (69, 581), (5, 37), (5, 21), (5, 6), (256,), (1, 256), (1, 639)}
