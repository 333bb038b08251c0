"""The steered-attention table (tests/steer_models.py) on the CPU oracle: what tests/test_gpu_steered_attention.py compares the
device with is decided by the rejection rule and not by rounding -- the float32 and the float64 search agree on every string, length,
rejection position, count and on every alignment row's non-zero pattern, with no exclusion --, `search` yields what
oracle.decode.decode_sequence_beam yields (which raises IndexError on the beyond-the-line cases, and only there), every promise of
the table is met by the trace -- the misalignments 2/21, 1/9 and 1/8 among them --, and each of the four flipped rules and of the
two moved thresholds (0.09, 0.13) changes the output the table names."""
import numpy as np
import pytest

from oracle.decode import decode_sequence_beam
from tests.lm_oracle import decode_sequence_beam_lm
from tests.steer_models import CASES, BY_NAME, REJECTION_RULES, THRESHOLD_RULES, run_search, steered_weights, track, GATE_OFF
from tests.tie_models import uniform_weights

TRACE_KEYS = ('rej_mis_inside', 'rej_mis_outside', 'half_down', 'half_up', 'is1_by_attention', 'is1_by_rejection', 'beyond_line',
              'zero_source_row')
_runs = {}


def _run(case, dtype=np.float32, rules=()):
    key = (case.name, np.dtype(dtype).name, tuple(rules))
    if key not in _runs:
        _runs[key] = run_search(case, dtype, rules)
    return _runs[key]


def _outputs(run):
    """The named outputs of a run over all lines and results."""
    return dict(text=[[r[0] for r in res] for res, _, _ in run], rej=[[list(r[4]) for r in res] for res, _, _ in run],
                n_found=[st['finals'] for _, st, _ in run], n_steps=[st['steps'] for _, st, _ in run])


def _patterns(res):
    return [[tuple(np.flatnonzero(np.asarray(a))) for a in r[3]] for r in res]


def test_the_gate_track_gives_exact_rows_in_both_precisions():
    """exp(G tanh(GATE_OFF)) is exactly 0 and exp(G tanh(0)) exactly 1, in float32 and in float64."""
    case = BY_NAME['mis_2_21']
    for dt in (np.float32, np.float64):
        m = case.model(dt)
        enc = case.encoder_outputs(m)
        _, st = m.step(np.zeros((1, case.V), dt), enc[0], enc[1:])
        assert st[-1].dtype == dt
        want = case.expected_row(0, case.a0[0] + 1).astype(dt) if dt == np.float32 else None
        a = st[-1][0]
        inside = [s for s in case.allowed[0] if abs(case.a0[0] + 1 - s) <= case.window]
        assert list(np.flatnonzero(a)) == inside and len(set(a[inside])) == 1 and a[inside[0]] == dt(1) / dt(len(inside))
        if want is not None:
            assert np.array_equal(a.view(np.int32), want.view(np.int32))
    w = steered_weights(case.cfg, uniform_weights(case.cfg))
    assert np.count_nonzero(w['att_U']) == 1 and np.count_nonzero(w['att_va']) == 1 and not w['att_Wa'].any()
    assert list(track(5, [1, 3])) == [GATE_OFF, 0, GATE_OFF, 0, GATE_OFF]


@pytest.mark.parametrize('name', [c.name for c in CASES])
def test_float32_and_float64_agree_without_exclusions(name):
    case = BY_NAME[name]
    for (r32, s32, _), (r64, s64, _) in zip(_run(case), _run(case, np.float64)):
        assert s32 == s64
        assert [r[0] for r in r32] == [r[0] for r in r64]
        assert [list(r[4]) for r in r32] == [list(r[4]) for r in r64]
        assert _patterns(r32) == _patterns(r64)


@pytest.mark.parametrize('name', [c.name for c in CASES])
def test_search_is_the_oracle_and_the_oracle_raises_beyond_the_line_only(name):
    case = BY_NAME[name]
    m = case.model()
    enc_in = case.inputs(m)[0]
    enc = case.encoder_outputs(m)
    raised = 0
    for j, (res, stats, trace) in enumerate(_run(case)):
        got = {}
        decode = decode_sequence_beam_lm if case.lm else decode_sequence_beam
        try:
            want = list(decode(m, source_seq=enc_in[j], encoder_outputs=[e[j:j + 1] for e in enc], stats=got))
        except IndexError:
            assert trace['beyond_line'] > 0
            raised += 1
            continue
        assert trace['beyond_line'] == 0 and got == stats and len(want) == len(res)
        for a, b in zip(want, res):
            assert a[0] == b[0] and a[2] == b[2] and np.array_equal(np.asarray(a[1]), np.asarray(b[1]))
            assert all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))
    assert bool(raised) == case.beyond


@pytest.mark.parametrize('name', [c.name for c in CASES])
def test_the_promises_of_the_table_are_met(name):
    case = BY_NAME[name]
    total = {k: sum(tr[k] for _, _, tr in _run(case)) for k in TRACE_KEYS}
    for key, promise in case.promises.items():
        assert key in TRACE_KEYS, key
        assert (total[key] > 0) if promise else (total[key] == 0), (key, total)
    # the misalignments the case is named after occur, in both precisions (fl32(1/k) rows: to 1e-6)
    for dtype in (np.float32, np.float64):
        traces = [tr for _, _, tr in _run(case, dtype)]
        if case.mis_inside is not None:
            assert abs(max(tr['mis_inside_max'] for tr in traces if tr['mis_inside_max'] is not None) - case.mis_inside) < 1e-6
        if case.mis_outside is not None:
            assert abs(min(tr['mis_outside_min'] for tr in traces if tr['mis_outside_min'] is not None) - case.mis_outside) < 1e-6
    for res, _, _ in _run(case):
        for r in res:
            # a rejection step's alignment is one-hot at its position, and the string shows the source character there
            for s, pos in enumerate(r[4]):
                if pos >= 0:
                    assert np.array_equal(r[3][s], np.eye(case.T, dtype=np.float32)[pos])


@pytest.mark.parametrize('name,rule', [(c.name, rule) for c in CASES for rule in c.flips])
def test_a_flipped_rule_changes_the_named_output(name, rule):
    case = BY_NAME[name]
    base, flipped = _outputs(_run(case)), _outputs(_run(case, rules=(rule,)))
    assert base[case.flips[rule]] != flipped[case.flips[rule]], (name, rule)


def test_the_table_reaches_every_branch_and_every_width():
    for key in TRACE_KEYS:
        assert any(c.promises.get(key) for c in CASES), key
    for rule in REJECTION_RULES + THRESHOLD_RULES:
        assert any(rule in c.flips for c in CASES), rule
    assert any(c.mis_inside for c in CASES) and sum(c.mis_outside is not None for c in CASES) >= 2
    assert {c.window for c in CASES} == {1, 2, 3, 4, 5}
    assert {c.N for c in CASES} >= {1, 4, 8, 64}
    assert any(c.lm for c in CASES) and any(c.family != 'uniform' for c in CASES)
    assert all(24 <= c.T + c.open_end <= 40 and 16 <= c.V <= 64 for c in CASES)
