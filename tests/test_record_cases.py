"""tests/record_cases.py on the CPU: the fp32 oracle yields what the case table promises, `expected_records` agrees with the host
path (sharding.records_from_lines on the oracle's strings) in every word but the greedy score, every mutation of it changes a
record of the table, and the host path's greedy score is measured against the float64 restatement."""
import math

import numpy as np
import pytest

from cor_asv_ann_amd import sharding
from oracle.decode import correct_lines, decode_batch_greedy
from tests.record_cases import (BY_NAME, CASES, C_I, CH_A, CHUNK_COUNTS, EOS, HOST_SCORE_BOUND, HOST_SCORE_MEASURED, I_C, MUTATIONS, V,
                                VARIANTS, dense, expected_records, first_eos, nonpad, oracle_of, oracle_out)


def _host_model():
    """The facade without a device: its host-side tables and bookkeeping only."""
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence
    s2s = Sequence2Sequence()
    s2s.mapping, s2s.voc_size = (C_I, I_C), V
    s2s._eos = EOS
    return s2s


def test_the_oracle_yields_what_the_table_promises():
    gap = np.inf
    for case in CASES:
        g, b = oracle_of(case)
        gap = min(gap, g['gap'])
        live = nonpad(case.idx, case.val)
        if case.kind == 'greedy':
            assert [n is not None for n in case.counts] == list(live), case.name
            for steps in case.steps:
                S = case.S(steps)
                got = first_eos(g['idx'][:, :S], EOS)
                for j, want in enumerate(case.planned_eos(S)):
                    assert want is None or got[j] == want, (case.name, steps, j, got[j], want)
        else:
            assert [bool(n) for n in b['n_found']] == case.found, (case.name, b['n_found'])
            assert [bool(n) for n in b['len'][::case.max_results]] == case.found
            if case.max_results > 1:        # the results of a line differ, so that taking another one shows
                assert all(b['len'][r] > 0 for r in range(len(b['len']))) and len({t for ts in b['texts'] for t in ts[:4]}) > 3
    print('smallest logit gap between the winner and the runner-up over all steps of all cases: %.3f' % gap)
    assert gap >= 0.5
    # the counts reach both sides of the 64-lane ballot chunks, and the beam returns a..a\n
    assert {63, 64, 65, 127, 128, 129} <= set(CHUNK_COUNTS)
    assert [ts[0] for ts in oracle_of(BY_NAME['beam_found'])[1]['texts']] == [CH_A * n + '\n' for n in (3, 10, 40)]


@pytest.mark.parametrize('name', ['greedy_short', 'greedy_confmat'])
def test_the_restated_greedy_loop_is_the_oracles(name):
    case = BY_NAME[name]
    want = decode_batch_greedy(case.model(), dense(case.idx, case.val), return_indexes='probs')
    got = oracle_of(case)[0]
    assert np.array_equal(got['idx'], want[5]) and np.array_equal(got['prob'], want[6].astype(np.float32))


@pytest.mark.parametrize('name,steps', [(n, s) for n, s in VARIANTS if BY_NAME[n].lines is not None])
def test_expected_records_agree_with_the_host_path(name, steps):
    """The host path: the oracle's strings, probability lists and scores through sharding.records_from_lines."""
    case = BY_NAME[name]
    S = case.S(steps)
    m = case.model()
    lut = _host_model()._codepoint_lut()
    if case.kind == 'greedy':
        _, lines, probs, scores, _ = decode_batch_greedy(m, dense(case.idx, case.val))
    else:
        lines, probs, scores, _ = correct_lines(m, case.lines, case.conf, fast=False, greedy=False)
    host = sharding.records_from_lines(lines, probs, scores, lut, S)
    want = expected_records(case.idx, case.val, oracle_out(case, steps), EOS, S)
    words = np.ones(2 * S + 4, bool)
    if case.kind == 'greedy':
        words[2 * S + 1:2 * S + 3] = False
        cut = [n is not None and n >= S for n in case.counts]       # (the oracle's score of a line cut at S is over its 2T steps)
        a, b = sharding.unpack_records(host)[3], sharding.unpack_records(want)[3]
        assert np.allclose(a[~np.array(cut)], b[~np.array(cut)], rtol=1e-6, atol=0)
    assert np.array_equal(host[:, words], want[:, words]), name


def test_every_mutation_changes_a_record_of_the_table():
    changed = {}
    for name, steps in VARIANTS:
        case = BY_NAME[name]
        S = case.S(steps)
        out = oracle_out(case, steps)
        want = expected_records(case.idx, case.val, out, EOS, S)
        for mut in MUTATIONS:
            got = expected_records(case.idx, case.val, out, EOS, S, mutate=mut)
            if not np.array_equal(got, want):
                changed.setdefault(mut, []).append((name, steps))
    for mut in MUTATIONS:
        print(mut, changed.get(mut))
    assert set(changed) == set(MUTATIONS), sorted(set(MUTATIONS) - set(changed))


def test_the_greedy_score_of_the_host_path():
    """Sequence2Sequence._greedy_results takes -np.log of the float32 probabilities in float32 and sums in float64; the record's
    score is the float64 restatement.  Every term is non-negative, so the sum's relative error is at most the worst term's: a few
    float32 ulp of numpy's log.  The measured value stands in tests/record_cases.py; the bound is twice that, at most 8 * 2**-24."""
    s2s = _host_model()
    worst = 0.0
    for case in CASES:
        if case.kind != 'greedy':
            continue
        live = nonpad(case.idx, case.val)
        for steps in case.steps:
            S = case.S(steps)
            out = oracle_out(case, steps)
            _, _, scores, _ = s2s._greedy_results(out['idx'], out['prob'], None, live)
            n = np.where(first_eos(out['idx'], EOS) >= 0, first_eos(out['idx'], EOS) + 1, S)
            for j in np.flatnonzero(live):
                want = math.fsum(-math.log(float(p)) for p in out['prob'][j, :n[j]]) / n[j]
                if want == 0:               # (every probability of the line is fl32(1.0))
                    assert scores[j] == 0
                    continue
                worst = max(worst, abs(scores[j] - want) / want)
    print('largest relative difference of the host path\'s greedy score from the float64 restatement: %.3e = %.2f * 2**-24'
          % (worst, worst * 2 ** 24))
    assert HOST_SCORE_BOUND == min(2 * HOST_SCORE_MEASURED, 8 * 2.0 ** -24)
    assert worst <= HOST_SCORE_BOUND
