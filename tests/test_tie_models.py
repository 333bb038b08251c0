"""The tie models' case table (tests/tie_models.py), checked on the CPU: what tests/test_gpu_beam_ties.py compares the device with
is well-conditioned, really made of ties, reaches every launch form of the beam kernels, and would change if an order rule did."""
import numpy as np
import pytest

from oracle.decode import decode_sequence_beam
from tests.lm_oracle import decode_sequence_beam_lm
from tests.tie_models import CASES, BY_NAME, RULES, beam_form, run_search, groups_of

_runs = {}


def _run(case, dtype=np.float32, rules=(), lm=False):
    key = (case.name, np.dtype(dtype).name, tuple(rules), lm)
    if key not in _runs:
        _runs[key] = run_search(case, dtype, rules, lm)
    return _runs[key]


def _decisions(run):
    """What must be equal between two searches of a case: per line every result's string, length and rejection positions, and the
    counts of finished hypotheses and of steps."""
    return [([(r[0], len(r[0]), tuple(r[4])) for r in res], stats['finals'], stats['steps']) for res, stats, _ in run]


def _sum(case, key):
    return sum(tr[key] for _, _, tr in _run(case))


def _max(case, key):
    return max(tr[key] for _, _, tr in _run(case))


VARIANTS = [(c.name, False) for c in CASES] + [(c.name, True) for c in CASES if c.lm]


@pytest.mark.parametrize('name,lm', VARIANTS)
def test_the_search_with_no_rule_flipped_is_the_oracle(name, lm):
    """`search` (the copy with switches and a trace) against oracle.decode.decode_sequence_beam, and with lm_predict against
    tests/lm_oracle.py decode_sequence_beam_lm: strings, probabilities, scores and alignments bit for bit, the stats, the LM
    oracle's rejection positions."""
    case = BY_NAME[name]
    m = case.model()
    enc_in, _ = case.inputs(m)
    enc = m.encode(enc_in)
    oracle = decode_sequence_beam_lm if lm else decode_sequence_beam
    for j, (res, stats, _) in enumerate(_run(case, lm=lm)):
        ostats = {}
        want = list(oracle(m, source_seq=enc_in[j], encoder_outputs=[e[j:j + 1] for e in enc], stats=ostats))
        assert ostats == stats
        assert len(want) == len(res)
        for a, b in zip(res, want):
            assert a[0] == b[0] and a[2] == b[2]
            assert np.array_equal(np.asarray(a[1], np.float32).view(np.int32), np.asarray(b[1], np.float32).view(np.int32))
            assert np.array_equal(np.asarray(a[3]), np.asarray(b[3]))
            if lm:
                assert list(a[4]) == list(b[4])


@pytest.mark.parametrize('name,lm', VARIANTS)
def test_every_case_is_decided_by_the_rules_not_by_rounding(name, lm):
    """No exclusions: the fp32 and the fp64 search agree on every result of every line; and every variant pops tied nodes."""
    case = BY_NAME[name]
    assert _decisions(_run(case, lm=lm)) == _decisions(_run(case, np.float64, lm=lm))
    assert all(len(res) == stats['finals'] for res, stats, _ in _run(case, lm=lm))
    if lm:
        assert sum(tr['tied_pops'] for _, _, tr in _run(case, lm=True)) >= 1


def test_the_models_are_what_they_claim():
    for case in CASES:
        w = case.weights()
        if case.family == 'uniform':
            assert all(not v.any() for v in w.values())
            continue
        g = groups_of(case.V, case.family[1], case.family[2])
        for v in range(case.V):
            assert np.array_equal(w['E'][v], w['E'][int(np.flatnonzero(g == g[v])[0])])
        assert len(np.unique(w['E'].sum(axis=1))) > 1
        assert (g[0] != g[1]) == bool(case.family[2]) and (g == g[0]).sum() > 1 and (g == g[1]).sum() > 1
        assert all(not w[k].any() for k in w if k != 'E' and not k.endswith('_b'))
        # the source characters of the first line lie in one group
    h4 = BY_NAME['h4_v24_n4']
    assert len(set(groups_of(24, 4, True)[h4.lines[0]])) == 1
    # sigmoid(30) is 1 and 0.5 * tanh(0) is 0 in float32: the state is held
    assert np.float32(1) / (np.float32(1) + np.exp(np.float32(-30))) == np.float32(1)


def test_the_ties_are_real():
    """Every case pops two distinct nodes of equal pro_cost one after the other -- except the edges that cannot hold two nodes at
    all (no_ties below, each with its reason); the cases named for a cut have the cut between two equal keys; the promises about
    the rejection candidate and the final list hold."""
    no_ties = {'u_v2_n4': 'V = 2: the only child is the newline', 'u_v65_t1': 'T = 1 with beam_width_in = 1: one child',
               'u_thr_above': 'the threshold one ulp above the tied score leaves the rejection candidate alone'}
    for case in CASES:
        tied = _sum(case, 'tied_pops')
        if case.name in no_ties:
            assert tied == 0 and _max(case, 'queue_max') <= 1, case.name
        else:
            assert tied >= 1, case.name
        p = case.promises
        if p.get('cut') == 'width':
            assert _sum(case, 'width_cut_ties') >= 1, case.name
        if p.get('cut') == 'cap':
            assert _sum(case, 'cap_cut_ties') >= 1 and _max(case, 'queue_max') > case.form['q_cap'], case.name
        if p.get('behind'):
            assert _sum(case, 'rej_behind') >= 1, case.name
        if p.get('rej0'):
            assert _sum(case, 'rej_index0') >= 1, case.name
        if p.get('many_finals'):
            assert _max(case, 'finals_per_pop_max') > case.form['pop_cap'] - case.N == 64, case.name
        if p.get('over_f_cap'):
            assert _max(case, 'finals_max') > 64, case.name
        if 'big_sort' in p:
            assert (_max(case, 'new_keys_max') > 4096) == p['big_sort'], case.name
            assert not p['big_sort'] or _max(case, 'new_keys_max') > case.form['sort_cap']
        if 'staged' in p:
            assert case.form['staged'] == p['staged'], case.name
    assert sum(_sum(c, 'rej_inside') > 0 for c in CASES) > 5 and sum(_sum(c, 'rej_raised') > 0 for c in CASES) > 5
    # the rejection threshold at and one ulp below the tied score raises nothing, one ulp above it does
    assert _sum(BY_NAME['u_rej_eq'], 'rej_raised') == 0 == _sum(BY_NAME['u_rej_below'], 'rej_raised') < _sum(BY_NAME['u_rej_above'], 'rej_raised')
    # the relative threshold: at the tied score and below it the ties stay in the beam, one ulp above they all leave
    assert _decisions(_run(BY_NAME['u_thr_eq'])) == _decisions(_run(BY_NAME['u_thr_below'])) != _decisions(_run(BY_NAME['u_thr_above']))


def test_the_table_reaches_every_form():
    """The launch forms of csrc/beam_kernels.hip, computed by tie_models.beam_form (which restates beam_lds_bytes and
    launch_beam_step), and the parameter values the table is to cover."""
    forms = {c.name: c.form for c in CASES}
    reached = {(f['waves'], f['split'], f['VPL']) for f in forms.values()}
    want = {(4, False, v) for v in (4, 8, 16, 32, 64)} | {(8, False, v) for v in (4, 8, 16, 32, 64)} | {(16, True, v) for v in (4, 8, 16)}
    assert reached == want                               # (16 waves exist only with the split phase A, up to VPL 16)
    assert {(8, False, 32)} <= {(f['waves'], f['split'], f['VPL']) for c, f in ((c, c.form) for c in CASES) if c.N >= 64}
    assert {c.N for c in CASES} >= {1, 3, 4, 8, 16, 64, 256}
    assert {c.V for c in CASES} >= {2, 65, 4096} and any(c.V <= 256 for c in CASES)
    assert {c.width_in for c in CASES} >= {1, 3, 15, 50} and any(c.width_in >= c.V for c in CASES)
    assert {c.width_out for c in CASES} >= {1, 4, 16, 63}
    assert {c.T for c in CASES} >= {1, 2} and any(len(set(map(len, c.lines))) > 1 for c in CASES)
    assert any(all(v == 0 for v in line) and line for c in CASES for line in c.lines)          # a line of unmapped characters
    assert {c.rejection for c in CASES} >= {0.0, 1.0}
    for split in (False, True):
        sel = [c for c in CASES if c.form['split'] == split]
        assert {c.form['staged'] for c in sel} == {True, False}
        assert {bool(c.promises.get('big_sort')) for c in sel} == {True, False}
        assert any(c.promises.get('cut') == 'cap' for c in sel) and any(c.promises.get('many_finals') for c in sel)
        assert any(c.lm for c in sel)
    assert all(c.T <= 12 for c in CASES if c.N >= 256)
    # beam_form against figures read off the kernel source by hand: N = 256 cuts the sort capacity to 2048 keys (7 * 257 * 4 + 320 * 16
    # + 4096 * 12 bytes exceed 56 KiB), N = 8 with 16 children sorts 128 at once
    assert beam_form(256, 96, 50, 3)['sort_cap'] == 2048 and beam_form(8, 64, 15, 5)['sort_cap'] == 128
    assert beam_form(64, 64, 50, 2)['staged'] and not beam_form(64, 64, 50, 3)['staged']


SMALL = [c for c in CASES if c.N <= 16 and c.V <= 100]


@pytest.mark.parametrize('rule', RULES)
def test_a_flipped_rule_changes_an_expected_output(rule):
    """The comparison can fail: with one order rule flipped the search returns something else on at least one case."""
    changed = [c.name for c in SMALL if _decisions(_run(c, rules=(rule,))) != _decisions(_run(c))]
    print('%s changes %d of %d cases: %s' % (rule, len(changed), len(SMALL), changed))
    assert changed
