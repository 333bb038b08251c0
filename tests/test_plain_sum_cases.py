"""The cases and the comparator of tests/test_gpu_plain_sums.py, tested on the CPU (tests/plain_sum_cases.py): every run plans to the
forms, shares and clears of the table; float32 arithmetic as the kernels form the sum passes the comparator on every case (the
project's bounds are not tighter than float32 itself, K = 4128 and 10272 included); every mutant of the reference fails it wherever
it applies; and the table of forms and fields names a run for every pair it calls held."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import lstm_gemm_cases as lg
from tests import plain_sum_cases as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def cases():
    return ps.build_cases()


def _runs(cases):
    for case in cases.values():
        for run in case.runs:
            yield case, run


def test_the_cases_are_what_the_issue_lists(cases):
    shapes = {name: (c.job.M, c.job.N, sum(s.width for s in c.job.segs)) for name, c in cases.items()}
    assert shapes == {'edge': (300, 198, 1024), 'uneven': (300, 198, 1568), 'short_last': (44, 96, 4128), 'empty_share': (44, 96, 10272),
                      'segments': (300, 198, 1024), 'natural_2wg': (1100, 390, 1024), 'natural_mid': (2048, 512, 2048),
                      'cut32': (8300, 1024, 64), 'cut64': (12392, 1024, 64), 'cut256': (8492, 2048, 64)}
    assert set(ps.RUNS) == set(cases)
    strides = {name: (c.job.segs[0].pool.shape[2], c.job.out[1]) for name, c in cases.items()}
    assert strides['edge'] == (1024 + 32, 232) and strides['cut32'] == strides['cut64'] == (96, 1056) and strides['cut256'] == (96, 2080)
    assert all(c.strided for c in cases.values())
    seg = cases['segments'].job
    assert [(s.width, s.koff) for s in seg.segs] == [(480, 544), (320, 224), (224, 0)] and all(s.rows is not None for s in seg.segs)
    assert all(s.rows is None for name, c in cases.items() if name != 'segments' for s in c.job.segs)
    for name in ('edge', 'uneven'):             # every form plain, with accumulate, with out_zeroed and with bias null
        labels = {r.label for r in cases[name].runs}
        for form in ('k32', 'g128', 'g128x2', 's128_mode1', 's128_mode2'):
            assert {form, form + '_acc', form + '_zeroed', form + '_nobias'} <= labels, (name, form)
    for name, c in cases.items():               # every case plain and with accumulate; one label, one run
        labels = [r.label for r in c.runs]
        assert len(set(labels)) == len(labels)
        assert any(r.fields['accumulate'] for r in c.runs) and any(not r.fields['accumulate'] for r in c.runs), name
    # the shares the module's text speaks of
    assert [b - a for a, b in ps.share_ranges(1568, 16, 6)] == [17 * 16] * 5 + [13 * 16]
    assert [b - a for a, b in ps.share_ranges(4128, 16, 16)][-2:] == [17 * 16, 3 * 16]
    assert [b - a for a, b in ps.share_ranges(10272, 16, 40)][-3:] == [13 * 16, 0, 0]
    assert [b - a for a, b in ps.share_ranges(4128, 32, 16)][-2:] == [3 * 32, 0]
    assert [b - a for a, b in ps.share_ranges(10272, 32, 40)][-5:] == [6 * 32, 0, 0, 0, 0]
    assert ps.share_ranges(1024, 16, 4) == [(0, 256), (256, 512), (512, 768), (768, 1024)]       # (segments: borders at 480 and 800)


def test_pools_hold_nan_wherever_no_index_points(cases):
    for c in cases.values():
        for sg in c.job.segs:
            slots, pool_rows, ld = sg.pool.shape
            assert pool_rows > c.job.M and ld > sg.width and np.isnan(sg.pool[:, :, sg.width:]).all()
            named = np.zeros(pool_rows, bool)
            named[sg.rows if sg.rows is not None else np.arange(c.job.M)] = True
            slot = sg.slot(c.step)
            assert np.isnan(sg.pool[slot, ~named]).all() and np.isfinite(sg.pool[slot, named, :sg.width]).all()
            assert all(np.isnan(sg.pool[s]).all() for s in range(slots) if s != slot)
        assert np.isfinite(c.C0).all() and 0.9 < c.C0.std() < 1.1
        z = c.base().z
        assert 0.9 < z.std() < 1.1, (c.name, z.std())                               # the product has unit deviation


def test_the_reference_is_the_plain_float64_sum(cases):
    c = cases['segments']
    A, Bt, order = c.operands()
    assert sorted(order) == list(range(1024)) and list(order[:3]) == [544, 545, 546]
    for run in c.runs[:2]:
        ref = c.reference(run)
        want = A @ Bt.T + c.job.bias + (c.C0 if run.fields['accumulate'] else 0)
        assert np.allclose(ref.z, want, rtol=0, atol=1e-12)
        mag = np.abs(A) @ np.abs(Bt).T + np.abs(c.job.bias) + (np.abs(c.C0) if run.fields['accumulate'] else 0)
        assert np.allclose(ref.mag, mag, rtol=1e-12)
    assert passes_exact(c, c.runs[0])


def passes_exact(case, run):
    ref = case.reference(run)
    return ps.passes(ref.z.astype(np.float32), ref)


# ---- (a) plans ----
@pytest.fixture(scope='module')
def planned(cases, tmp_path_factory):
    """{(case, label): (plan, clears)} as tests/gemm_plan_driver.cpp plans the runs at 256 CUs"""
    cxx = os.environ.get('CXX') or next((c for c in ('c++', 'g++', 'clang++') if shutil.which(c)), None)
    if not cxx or not shutil.which(cxx):
        pytest.skip('no host compiler')
    exe = str(tmp_path_factory.mktemp('plain_sum_plan') / 'driver')
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', os.path.join(ROOT, 'tests', 'gemm_plan_driver.cpp'), '-o', exe], check=True)
    text = ''.join(ps.plan_line(c, r) + '\n' for c, r in _runs(cases))
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    recs, name = {}, None
    for line in out.splitlines():
        if line.startswith('case '):
            name = line[5:]
            recs[name] = []
        else:
            recs[name].append(line)
    got = {}
    for c, r in _runs(cases):
        lines = recs['%s_%s' % (c.name, r.label)]
        plan = [(rec.split()[1], int(re.search(r'grid=\d+,\d+,(\d+)', rec).group(1))) for rec in lines if rec.startswith('L ')]
        got[c.name, r.label] = (plan, sum(rec.startswith('C ') for rec in lines), lines)
    return got


def test_every_run_plans_to_the_forms_shares_and_clears_of_the_table(cases, planned):
    for c, r in _runs(cases):
        plan, clears, _ = planned[c.name, r.label]
        assert plan == r.plan and clears == r.clears, (c.name, r.label, plan, clears)
        # a clear there is exactly where partial sums meet in atomics on a C nobody prepared
        assert clears == int(r.shares > 1 and not (r.fields['accumulate'] or r.fields['out_zeroed']))
    # the cuts: the head's rows, and the tail's pointers moved by rows * ld (not by rows * width)
    for name in ('cut32', 'cut64', 'cut256'):
        c = cases[name]
        _, _, lines = planned[name, 'cut_acc' if name != 'cut256' else 'cut']
        rows = [int(m) for rec in lines for m in re.findall(r'\| M=(\d+)', rec)]
        assert rows == [ps.CUT_ROWS[name], c.job.M - ps.CUT_ROWS[name]]
        a0 = [int(re.search(r' a0=([0-9a-f]+)/', rec).group(1), 16) for rec in lines]
        o = [int(re.search(r' o=([0-9a-f]+) ', rec).group(1), 16) for rec in lines]
        assert a0[1] - a0[0] == 4 * ps.CUT_ROWS[name] * c.job.segs[0].pool.shape[2] and o[1] - o[0] == 4 * ps.CUT_ROWS[name] * c.job.out[1]


def test_the_table_of_forms_and_fields_names_a_run_for_every_pair_it_holds(cases):
    assert set(ps.HELD) == {(form, field) for form in ps.FORMS for field in ps.FIELDS}
    for (form, field), word in ps.HELD.items():
        holders = [(c.name, r.label) for c, r in _runs(cases) if ps.run_has(c, r, form, field)]
        if word == 'held':
            assert holders, (form, field)
        else:
            assert word.startswith('never: ') and not holders, (form, field, holders)
    for form in ps.FORMS:
        assert ('%-13s' % ('  ' + form)) in ps.__doc__


# ---- (b) the comparator is not too tight ----
def test_float32_sums_as_the_kernels_form_them_pass_the_comparator(cases):
    rng = np.random.default_rng(7)
    for c in cases.values():
        seen = set()
        for r in c.runs:
            key = (r.plan[0], r.bias, r.fields['accumulate'])
            if key in seen or (r.shares == 1 and r.plan[0][0] not in ('g128', 's256')):         # (one chain over all of K: once per case)
                continue
            seen.add(key)
            ref = c.reference(r)
            rms, mx = lg.plain_errors(ps.emulate(c, r, rng), ref)
            assert rms < ps.RMS_BOUND and mx < ps.MAX_BOUND, (c.name, r.label, rms, mx)
    # ... and the longest chains there are: all of K = 4128 and 10272 in one share
    for name in ('short_last', 'empty_share'):
        c = cases[name]
        r = c.runs[0]
        rms, mx = lg.plain_errors(ps.emulate(c, r, rng, shares=1), c.reference(r))
        assert rms < ps.RMS_BOUND and mx < ps.MAX_BOUND, (name, rms, mx)


# ---- (c) mutants ----
SMALL = {'edge', 'uneven', 'short_last', 'empty_share', 'segments', 'natural_2wg', 'natural_mid'}
CUTS = {'cut32', 'cut64', 'cut256'}
APPLIES = {'bias_by_every_share': SMALL, 'last_share_dropped': SMALL, 'first_tile_twice': SMALL, 'c0_ignored': SMALL | CUTS, 'c0_twice': SMALL | CUTS,
           'second_group_dropped': {'edge', 'uneven', 'short_last', 'empty_share', 'natural_2wg'},
           'empty_share_contracts': {'short_last', 'empty_share'},          # (short_last: the 16th share of the 32-row tiles)
           'tail_reads_a_with_k': CUTS, 'tail_writes_c_with_n': CUTS}


@pytest.mark.parametrize('name', sorted(SMALL | CUTS))
def test_every_mutant_fails_the_comparator_wherever_it_applies(cases, name):
    assert set(APPLIES) == set(ps.MUTANTS) and SMALL | CUTS == set(cases)
    c = cases[name]
    applied = set()
    for r in c.runs:
        if name in CUTS and r.label not in ('cut', 'cut_acc'):      # (the other runs of a cut case repeat these two's mutants: the test's time)
            continue
        ref = c.reference(r)
        if name in CUTS:                # (the head's first and last tile rows and the whole tail)
            ref.live = (np.arange(c.job.M) < 128) | (np.arange(c.job.M) >= ps.CUT_ROWS[name] - 128)
        assert ps.passes(ref.z.astype(np.float32), ref), (name, r.label)
        for m in ps.MUTANTS:
            got = ps.mutant(c, r, m)
            if got is None:
                continue
            applied.add(m)
            assert not ps.passes(got, ref), (name, r.label, m, lg.plain_errors(got, ref))
    assert applied == {m for m in ps.MUTANTS if name in APPLIES[m]}
