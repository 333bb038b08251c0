"""The train step's plain contractions in every launch form, against float64 (C ABI: casv_debug_gemm_jobs_sum -> launch_gemm_batch).

What csrc/train.hip's plain_gemm() sets and no other caller does -- ksplit = -1 (K shared out over workgroups, the partial sums added
with float atomics), kgroups = 2 (... and over the two wave groups of a workgroup), accumulate (C +=), out_zeroed, row strides
lda != K and ldc != N -- on the cases of tests/plain_sum_cases.py, in each form the planner makes of them: 128x128 fp32-input tiles,
the same on two wave groups, 32- and 64-row tiles, 128x128 and 256x256 split tiles; with one K share or several, with and without a
clear of C, with the cut of a partial round or of a ragged block behind them.  Per run: the statistics show the intended forms, shares
and clears; every element of rows < M and columns < N passes the comparator against float64 (the project's RMS_BOUND and MAX_BOUND);
every pad column, every other slot and the guard row is still 0xFF (the guard row is checked by the entry itself); launches of ONE
share agree bit for bit wherever the arithmetic says so.  Launches of several shares are compared with float64 only: their atomics
have no order."""
import copy
import time

import numpy as np
import pytest

from tests import lstm_gemm_cases as lg
from tests import plain_sum_cases as ps

pytestmark = pytest.mark.gpu

UNTOUCHED = np.uint32(0xFFFFFFFF)
CASES = ['edge', 'uneven', 'short_last', 'empty_share', 'segments', 'natural_2wg', 'natural_mid', 'cut32', 'cut64', 'cut256']
# Runs whose results must agree bit for bit: (labels, rows) -- rows: a slice of the rows that do (None: all).
#   every fp32-input tile shape contracts an element with the same k-ordered chain (ksplit 0, with and without accumulate);
#   ordered sums with ksplit -1 are the one-share launch of ksplit 0; out_zeroed changes nothing where there is one share;
#   the two split modes give the same bits; the cut forms equal the one-launch form.
#   cut256: the head is 256x256 split tiles in both runs; its tail keeps the fp32-input 32-row tiles (a launch that asks for split-K
#   does), so it equals the fp32-input launch of the whole job there, not the split one.
HEAD = slice(0, 8192)
TAIL = slice(8192, None)
SAME_BITS = {
    'edge': [(('one_g128', 'one_k32', 'one_k64', 'ordered_g128', 'ordered_k32', 'ordered_k32_natural', 'ordered_k64', 'one_k64_zeroed'), None),
             (('one_g128_acc', 'one_k32_acc', 'one_k64_acc'), None),
             (('one_s128_mode1', 'one_s128_mode2', 'ordered_s128_mode2'), None)],
    'cut32': [(('cut', 'one'), None), (('cut_acc', 'one_acc'), None)],
    'cut64': [(('cut', 'one'), None), (('cut_acc', 'one_acc'), None)],
    'cut256': [(('cut', 'cut_zeroed', 'cut_ordered'), None), (('cut', 'one'), HEAD), (('cut', 'one_fp32'), TAIL)],
}


@pytest.fixture(scope='module')
def cases():
    return ps.build_cases()


@pytest.fixture(scope='module')
def refs(cases):
    """the float64 reference of (case, bias, accumulate): computed once, shared, left unchanged"""
    memo = {}

    def ref(case, run):
        key = (case.name, run.bias, run.fields['accumulate'])
        if key not in memo:
            memo[key] = case.reference(run)
            memo[key].z.setflags(write=False)
            memo[key].mag.setflags(write=False)
        return memo[key]
    ref.drop = lambda name: [memo.pop(k) for k in list(memo) if k[0] == name]
    return ref


@pytest.fixture
def engine():
    from cor_asv_ann_amd.engine import HipEngine
    eng = HipEngine(1, 32, 8)
    try:
        yield eng
    finally:
        eng.set_option('split_bf16', -1)
        eng.set_option('tile', -1)
        eng.close()


def test_the_lists_name_every_case_and_run(cases):
    assert sorted(CASES) == sorted(cases) and set(SAME_BITS) <= set(cases)
    for name, groups in SAME_BITS.items():
        labels = {r.label: r for r in cases[name].runs}
        for group, _ in groups:
            assert set(group) <= set(labels), (name, group)
            assert all(labels[g].shares == 1 for g in group), (name, group)         # several shares: atomics without an order
            assert len({(labels[g].bias, labels[g].fields['accumulate']) for g in group}) == 1


def _launch(eng, case, run, step_by_ptr=False):
    """(slots, M, ld) of the run's output.  The statistics must show the intended forms, shares and clears."""
    eng.set_option('tile', run.tile)
    eng.set_option('split_bf16', run.arith)
    outs, forms, launches = eng.debug_gemm_jobs(0, [case.job_of(run)], case.step, step_by_ptr, sums=[case.sums_of(run)], ordered=run.ordered)
    shares = eng.stat('gemm_jobs_shares')
    got, want = (forms, launches, shares), (lg.form_mask(run.forms()), len(run.plan) + run.clears, run.shares)
    if got != want and eng.stat('cus') != 256:
        pytest.skip('this device has %d CUs, not 256: %s under %s plans to the forms %#x in %d shares, the case is meant for %s'
                    % (eng.stat('cus'), case.name, run.label, forms, shares, '+'.join('%s x%d' % p for p in run.plan)))
    assert got == want, (case.name, run.label, got, want)
    return outs[0]['out']


def _addressed(case, run, full):
    """(M, N) of the addressed slot; every other slot and every pad column must be untouched -- after a clear and with accumulate
    too -- and no element may be left unwritten"""
    job = case.job
    slots, ld, mul, add = job.out
    slot, bits = case.step * mul + add, full.view(np.uint32)
    assert full.shape == (slots, job.M, ld) and ld > job.N
    assert (bits[np.arange(slots) != slot] == UNTOUCHED).all(), (case.name, run.label, 'a store into another slot')
    assert (bits[slot][:, job.N:] == UNTOUCHED).all(), (case.name, run.label, 'a store into the pad columns')
    assert not (bits[slot][:, :job.N] == UNTOUCHED).any(), (case.name, run.label, 'an element was not written')
    return full[slot][:, :job.N]


def _run(eng, case, refs, run):
    t0 = time.perf_counter()
    full = _launch(eng, case, run)
    call = time.perf_counter() - t0
    got = _addressed(case, run, full)
    rms, mx = lg.plain_errors(got, refs(case, run))
    print('FIGURES %s %s: %s clears=%d rms=%.4f max=%.4f (call %.2f s)'
          % (case.name, run.label, '+'.join('%s x%d' % p for p in run.plan), run.clears, rms, mx, call))
    assert rms < ps.RMS_BOUND and mx < ps.MAX_BOUND, (case.name, run.label, rms, mx)
    return got


@pytest.mark.parametrize('name', CASES)
def test_case_in_every_form_against_float64(engine, cases, refs, name):
    case = cases[name]
    keep = {label for group, _ in SAME_BITS.get(name, []) for label in group}
    got = {}
    try:
        for run in case.runs:
            out = _run(engine, case, refs, run)
            if run.label in keep:
                got[run.label] = out.copy()
    finally:
        refs.drop(name)
    for group, rows in SAME_BITS.get(name, []):
        first = got[group[0]][rows or slice(None)].view(np.uint32)
        for label in group[1:]:
            assert np.array_equal(first, got[label][rows or slice(None)].view(np.uint32)), (name, '%s and %s differ in bits' % (group[0], label))


def test_ordered_sums_on_two_wave_groups_give_the_same_bits_every_time(engine, cases, refs):
    """what the deterministic train step runs: kgroups 2 under ordered sums -- one share, the wave groups added in a fixed order"""
    case = cases['edge']
    run = next(r for r in case.runs if r.label == 'ordered_g128x2')
    a, b = _run(engine, case, refs, run).copy(), _run(engine, case, refs, run)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_a_cleared_and_a_caller_zeroed_output_both_pass_and_the_latter_shows_no_clear(engine, cases, refs):
    for name in ('edge', 'uneven'):
        case = cases[name]
        for form in ('k32', 'g128', 'g128x2', 's128_mode2'):
            runs = {r.label: r for r in case.runs}
            plain, zeroed = runs[form], runs[form + '_zeroed']
            assert plain.shares > 1 and plain.plan == zeroed.plan
            _run(engine, case, refs, plain)
            assert engine.stat('gemm_jobs_launches') == 2 or engine.stat('cus') != 256           # the clear, then the launch
            _run(engine, case, refs, zeroed)
            assert engine.stat('gemm_jobs_launches') == 1 or engine.stat('cus') != 256


def test_the_step_through_a_device_word_goes_with_one_share_only(engine, cases, refs):
    """split-K clears the slot of the immediate step: a job that asks for it cannot take its step from a device word; with ksplit 0
    it can, accumulate included, and gives the bits of the immediate step"""
    case = cases['edge']
    runs = {r.label: r for r in case.runs}
    for label in ('one_g128', 'one_g128_acc', 'one_k32_acc'):
        imm = _addressed(case, runs[label], _launch(engine, case, runs[label]))
        ptr = _addressed(case, runs[label], _launch(engine, case, runs[label], step_by_ptr=True))
        assert np.array_equal(imm.view(np.uint32), ptr.view(np.uint32)), label


def test_bad_launch_fields_are_refused_before_anything_is_launched(engine, cases, refs):
    """Every condition of the entry's host checks is refused with CASV_ERR_ARG; the statistics of the last launch stay, and a valid
    call afterwards still works."""
    from cor_asv_ann_amd._native import NativeError
    case = cases['edge']
    runs = {r.label: r for r in case.runs}
    _run(engine, case, refs, runs['g128'])
    before = [engine.stat(k) for k in ('gemm_jobs_forms', 'gemm_jobs_launches', 'gemm_jobs_shares')]
    assert before == [1, 2, 4] or engine.stat('cus') != 256

    def refused(fields, epi=0, jobs=None, step=None, by_ptr=False, ordered=False, **change):
        jobs = jobs or [copy.copy(case.job)]
        for key, value in change.items():
            setattr(jobs[0], key, value)
        sums = [fields] + [None] * (len(jobs) - 1) if isinstance(fields, dict) else fields
        with pytest.raises(NativeError) as err:
            engine.debug_gemm_jobs(epi, jobs, case.step if step is None else step, by_ptr, sums=sums, ordered=ordered)
        assert err.value.code == -1, (fields, change, err.value)
        assert [engine.stat(k) for k in ('gemm_jobs_forms', 'gemm_jobs_launches', 'gemm_jobs_shares')] == before
    refused(dict(ksplit=-2))                                    # ksplit in [-1, 64]
    refused(dict(ksplit=65))
    refused(dict(kgroups=1))                                    # kgroups 0 or 2
    refused(dict(kgroups=3))
    refused(dict(kgroups=-2))
    refused(dict(accumulate=2, C0=case.C0))                     # the flags 0 or 1
    refused(dict(accumulate=-1))
    refused(dict(out_zeroed=2))
    refused(dict(accumulate=1, out_zeroed=1, C0=case.C0))       # not both
    refused(dict(ksplit=-1), by_ptr=True)                       # split-K and the step through a device word
    refused(dict(ksplit=4), by_ptr=True)
    # the four fields only on the plain-epilogue jobs of an epi = 0 batch
    rng = np.random.default_rng(5)
    cell = lg.make_job(rng, 130, 256, (32, 64, 32), (96, 32, 0), (2,))
    rider = lg.make_job(rng, 200, 96, (64,), (16,), (2,), Ktot=96, lstm=False, gather=(True,), epi_plain=True)
    for fields in (dict(ksplit=-1), dict(kgroups=2), dict(accumulate=1), dict(out_zeroed=1)):
        refused(fields, epi=1, jobs=[cell])
        refused([None, fields], epi=1, jobs=[cell, rider])
    # ... plus the checks of every jobs entry
    refused(dict(ksplit=-1), out=(4, 196, 1, 0))                # ld >= N
    refused(dict(ksplit=-1), step=4)                            # the slot lies outside the pools
    refused(dict(accumulate=1), step=4)
    refused(dict(ksplit=-1), Ktot=992, Bt=case.job.Bt[:, :992])          # koff + width <= Ktot
    engine.debug_gemm_jobs(1, [cell, rider], 2, sums=[None, None])      # (without a field the entry is the plain jobs entry)
    _run(engine, case, refs, runs['g128_acc'])
