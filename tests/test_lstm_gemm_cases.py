"""The comparator of tests/test_gpu_lstm_gemm.py, tested on the CPU (tests/lstm_gemm_cases.py): the float64 reference equals torch's
LSTMCell, float32 arithmetic passes the bounds, every wrong reading of the arguments does not, and every GPU case plans to the launch
form it is meant for."""
import re

import numpy as np
import pytest

from tests import gemm_plan_cases as gc
from tests import lstm_gemm_cases as lg
from tests.test_gemm_plan import planned          # noqa: F401  (the stand-alone driver of the planner, as a fixture)


@pytest.fixture(scope='module')
def cases():
    return lg.build_cases()


def _rows(job):
    """the rows the CPU tests compute: all of a small job, every 8th of a chip-filling one (and the pair `swap_rows` swaps)"""
    if job.M <= 2048:
        return None
    pairs = [m for sg in job.segs if sg.rows is not None for m in sg.swap_pair]
    return np.unique(np.concatenate([np.arange(0, job.M, 8), np.flatnonzero(job.live())[:64], pairs]).astype(np.int64))


def _runs(cases):
    for case in cases.values():
        for step in case.steps:
            for job in case.jobs:
                yield case, step, job


def test_the_cases_are_what_the_issue_lists(cases):
    small = cases['a_bias'].jobs[0]
    assert (small.M, small.N, small.Ktot) == (300, 256, 128) and [s.width for s in small.segs] == [32, 64, 32]
    assert all(s.pool.shape[2] == s.width + 32 for s in small.segs)
    assert [s.koff for s in small.segs] == [96, 32, 0]                              # K order differs from the order in memory
    assert [s.rows is not None for s in small.segs] == [True, True, False]
    assert cases['a_bias'].jobs[0].bias is not None and cases['a_nobias'].jobs[0].bias is None
    for name, mul in (('b_step_plus', 1), ('b_step_minus', -1)):
        job = cases[name].jobs[0]
        assert cases[name].steps == (3,) and all(s.step_mul == mul and s.step_add != 0 for s in job.segs + [job.c_in])
        assert job.c_out[2] * 3 + job.c_out[3] == 4                                 # slot step + 1
    job = cases['c_skip_first'].jobs[0]
    assert job.segs[1].skip_first and job.c_in.skip_first and cases['c_skip_first'].steps == (0, 1)
    job = cases['c_first_base'].jobs[0]
    assert job.segs[1].first is not None and job.segs[1].rows is not None and job.c_in.first is not None and job.c_in.rows is not None
    assert [j.M for j in cases['d_two_jobs'].jobs] == [300, 130]
    assert [(j.N, j.epi_plain) for j in cases['d_plain_rider'].jobs] == [(256, False), (96, True)]
    assert len(cases['d_four_jobs'].jobs) == 4
    for name, n2, live128 in (('e_straddle_dead', 32, False), ('e_straddle_live', 33, True)):
        job = cases[name].jobs[0]
        assert (job.M, job.nact_group, job.nact[2]) == (384, 48, n2) and job.live()[128] == live128 and not job.live()[129:256].any()
    job = cases['e_finished_lines'].jobs[0]
    assert (job.M, job.nact_group) == (1024, 256) and job.nact[1] == job.nact[3] == 0 and 1 in job.nact
    job = cases['f_side_outputs'].jobs[0]
    assert job.M == 300 and job.zinit is not None and job.gates_out and job.out2 and cases['f_side_outputs'].forms == lg.FP32_FORMS
    for name, M in (('s_8448', 8448), ('s_8492', 8492), ('s_8192_lines_of_8', 8192), ('s_8448_lines_of_8', 8448)):
        job = cases[name].jobs[0]
        assert (job.M, job.N, job.Ktot, len(job.segs)) == (M, 2048, 160, 3) and cases[name].steps == (0, 3)
        assert cases[name].forms == lg.SPLIT_FORMS and (job.nact_group == 8) == ('lines' in name)
    # the 256x256 kernel has its own copy of the step-0 forms and of the slot arithmetic: (c) first_base and (b) step addressing there
    job = cases['s_first_base'].jobs[0]
    assert (job.M, job.N) == (8448, 2048) and cases['s_first_base'].steps == (0, 3) and cases['s_first_base'].forms == lg.SPLIT_FORMS
    assert job.segs[1].first is not None and job.segs[1].rows is not None and job.c_in.first is not None and job.c_in.rows is not None
    job, rider = cases['s_step'].jobs
    assert (job.M, job.N) == (8448, 2048) and cases['s_step'].steps == (3,) and cases['s_step'].forms == lg.SPLIT_FORMS
    assert all(s.step_mul == -1 and s.step_add != 0 for s in job.segs + [job.c_in]) and job.out[2] == -1 and job.c_out[2] * 3 + job.c_out[3] == 4
    assert (rider.M, rider.N, rider.epi_plain) == (8192, 1024, True)
    assert all(c.forms == (lg.FP32_FORMS if n == 'f_side_outputs' else lg.ALL_FORMS) for n, c in cases.items() if not n.startswith('s_'))


def test_pools_hold_nan_wherever_no_index_points(cases):
    for case, step, job in _runs(cases):
        live = job.live()
        for part in job.segs + ([job.c_in] if job.c_in is not None else []):
            slots, pool_rows, ld = part.pool.shape
            assert pool_rows > job.M and ld > part.width
            assert np.isnan(part.pool[:, :, part.width:]).all()
            used = {s * part.step_mul + part.step_add for s in case.steps}
            for slot in range(slots):
                if slot not in used:
                    assert np.isnan(part.pool[slot]).all()
            named = np.zeros(pool_rows, bool)
            named[part.rows[live] if part.rows is not None else np.flatnonzero(live)] = True
            slot = part.slot(step)
            assert np.isnan(part.pool[slot, ~named]).all() and np.isfinite(part.pool[slot, named, :part.width]).all()
            if part.rows is not None:
                assert 0 <= part.rows.min() and part.rows.max() < pool_rows
                assert len(np.unique(part.rows[live])) < live.sum()                   # some rows repeat
                assert not (part.rows[live] == np.flatnonzero(live)).all()
                assert not named[part.rows[~live]].any()                              # dead rows name a NaN row
        rows = [tuple(p.rows) for p in job.segs + [job.c_in] if p is not None and p.rows is not None]
        assert len(set(rows)) == len(rows)                                            # every part its own index


def test_reference_equals_torch_lstm_cell(cases):
    torch = pytest.importorskip('torch')
    for case, step, job in _runs(cases):
        if not case.lstm(job) or job.M > 2048:
            continue
        ref = lg.reference(case, job, step)
        live = ref.live
        x = np.zeros((job.M, job.Ktot))
        for sg in job.segs:
            a = sg.read(step, job.M)
            if a is not None:
                x[:, sg.koff:sg.koff + sg.width] = a
        cp = job.c_in.read(step, job.M)
        cp = np.zeros((job.M, job.N // 4)) if cp is None else cp
        U = job.N // 4
        cell = torch.nn.LSTMCell(job.Ktot, U, bias=True, dtype=torch.float64)
        with torch.no_grad():
            # torch's gate order is i, f, g, o -- Keras' i, f, c~, o; the recurrent part is fed nothing: x carries [x | h | ctx]
            cell.weight_ih.copy_(torch.from_numpy(job.W.astype(np.float64).reshape(4 * U, job.Ktot)))
            cell.weight_hh.zero_()
            cell.bias_ih.copy_(torch.from_numpy((job.b if job.bias is not None else np.zeros_like(job.b)).astype(np.float64).reshape(4 * U)))
            cell.bias_hh.zero_()
            zin = 0 if job.zinit is None else job.zinit.read(step, job.M)[:, lg.gate_columns(U)].reshape(job.M, 4 * U)
            if job.zinit is None:
                h, c = cell(torch.from_numpy(x[live]), (torch.zeros(int(live.sum()), U, dtype=torch.float64), torch.from_numpy(cp[live])))
                assert np.abs(h.numpy() - ref.h[live]).max() <= 1e-12 and np.abs(c.numpy() - ref.c[live]).max() <= 1e-12, case.name
            else:       # (the precomputed term has no place in LSTMCell's interface: the same cell from its parts)
                z = torch.from_numpy(x[live]) @ cell.weight_ih.T + cell.bias_ih + torch.from_numpy(zin[live])
                i, f, g, o = z.chunk(4, 1)
                c = torch.sigmoid(f) * torch.from_numpy(cp[live]) + torch.sigmoid(i) * torch.tanh(g)
                h = torch.sigmoid(o) * torch.tanh(c)
                assert np.abs(h.numpy() - ref.h[live]).max() <= 1e-12 and np.abs(c.numpy() - ref.c[live]).max() <= 1e-12, case.name


def test_float32_arithmetic_passes_the_comparator(cases):
    """the bounds are not tighter than float32 arithmetic itself"""
    for case, step, job in _runs(cases):
        sel = _rows(job)
        ref = lg.reference(case, job, step, sel=sel)
        fig, ok = lg.judge(case, job, ref, lg.outputs_of(case, job, ref))
        assert ok and max(fig.values()) <= 1.0, (case.name, step, fig)                # float64 rounded to float32: at most 2^-24 |z| <= one unit
        f32 = lg.reference(case, job, step, dtype=np.float32, sel=sel)
        fig, ok = lg.judge(case, job, ref, lg.outputs_of(case, job, f32))
        assert ok, (case.name, step, fig)


def test_every_mutant_is_rejected_wherever_it_applies(cases):
    applied = {m: 0 for m in lg.MUTANTS}
    for case, step, job in _runs(cases):
        sel = _rows(job)
        ref = lg.reference(case, job, step, sel=sel)
        for mutant in lg.MUTANTS:
            wrong = lg.reference(case, job, step, mutant, sel=sel)
            if wrong is None:
                continue
            applied[mutant] += 1
            fig, ok = lg.judge(case, job, ref, lg.outputs_of(case, job, wrong))
            assert not ok, (case.name, step, mutant, fig)
    assert all(applied.values()), applied
    # where each must apply: the step-0 forms at step 0 only, the cell state's wherever it is read gathered
    c = cases['c_skip_first']
    assert lg.reference(c, c.jobs[0], 0, 'not_skipped') is not None and lg.reference(c, c.jobs[0], 1, 'not_skipped') is None
    assert lg.reference(c, c.jobs[0], 0, 'cprev_ungathered') is None and lg.reference(c, c.jobs[0], 1, 'cprev_ungathered') is not None
    assert lg.reference(c, c.jobs[0], 0, 'cprev_not_skipped') is not None and lg.reference(c, c.jobs[0], 1, 'cprev_not_skipped') is None
    for name in ('a_bias', 'b_step_minus', 'e_straddle_live', 'f_side_outputs'):
        assert all(lg.reference(cases[name], cases[name].jobs[0], cases[name].steps[0], m) is not None for m in lg.MUTANTS if 'not_skipped' not in m), name


def test_conditioning(cases):
    """A saturated cell would hide errors in z: fewer than 1 % of the pre-activations have |z| > 6; and every live output row is
    touched by a term a mutant moves: with one K tile dropped every live row has an element outside its bound."""
    for case, step, job in _runs(cases):
        sel = _rows(job)
        ref = lg.reference(case, job, step, sel=sel)
        z = ref.z[ref.live]
        assert np.isfinite(z).all() and (np.abs(z) > 6).mean() < 0.01 and 0.6 < z.std() < 1.5, (case.name, step, z.std())
        wrong = lg.outputs_of(case, job, lg.reference(case, job, step, 'drop_tile', sel=sel))
        if case.lstm(job):
            assert np.abs(ref.cprev[ref.live]).max() <= 2
            rc, rh = lg.cell_ratios(wrong['c_out'], wrong['out'], ref)
            bad = (rc > 1).any(axis=1) & (rh > 1).any(axis=1)
        else:
            err = np.abs(wrong['out'].astype(np.float64) - ref.z) / (ref.mag * lg.EPS)
            bad = (err > lg.MAX_BOUND).any(axis=1)
        assert bad[ref.live].all(), (case.name, step)


def _forms(records):
    return sorted({rec.split()[1] for rec in records if rec.startswith('L ')})


def test_every_gpu_case_plans_to_the_form_it_is_meant_for(cases, planned):        # noqa: F811
    """at 256 CUs; the GPU test reads the same from the statistic and skips a case, saying so, where another CU count plans otherwise"""
    lines = dict(gc.CASES)
    for case in cases.values():
        for form in case.forms:
            for step in case.steps:
                name = 'lstm_%s_%s_step%d' % (case.name, form, step)
                assert lines[name] == lg.plan_line(case, form, step, name), name
                assert _forms(planned[name]) == sorted(lg.intended_forms(case, form)), (name, planned[name])
                assert planned[name] == gc.EXPECTED[name]
    # the cut behind the whole rounds: 8192 rows as 256x256 tiles, the rest (a ragged block too) as 128x128 split tiles, and the
    # live-row counts move with a cut that falls on a line boundary
    for name, tail in (('s_8448', 256), ('s_8492', 300), ('s_8448_lines_of_8', 256), ('s_first_base', 256)):
        recs = gc.EXPECTED['lstm_%s_split2_image_step3' % name]
        assert [(r.split()[1], re.findall(r'\| M=(\d+)', r)) for r in recs] == [('s256', ['8192']), ('s128', [str(tail)])], recs
        assert 'img=1/1' in recs[0] and 'img=0/0' in gc.EXPECTED['lstm_%s_split2_staging_step3' % name][0]
    recs = gc.EXPECTED['lstm_s_step_split2_image_step3']         # two jobs as 256x256 tiles, one of them with the plain epilogue
    assert [(r.split()[1], re.findall(r'\| M=(\d+)', r), re.findall(r'ep=(\d)', r)) for r in recs] == \
        [('s256', ['8192', '8192'], ['0', '1']), ('s128', ['256'], ['0'])] and 'img=1/2' in recs[0], recs
    na = [re.search(r'na=(\w+)', r).group(1) for r in gc.EXPECTED['lstm_s_8448_lines_of_8_split2_image_step3']]
    assert int(na[1], 16) - int(na[0], 16) == 8192 // 8 * 4
    assert _forms(gc.EXPECTED['lstm_s_8192_lines_of_8_split2_image_step3']) == ['s256']
    # another CU count decides otherwise
    assert _forms(gc.EXPECTED['lstm_s_8448_split2_image_ncu304']) != _forms(gc.EXPECTED['lstm_s_8448_split2_image_step3'])
    # what a form cannot take, the planner refuses: the train step's side outputs never go as 256x256 tiles, and a small launch that
    # carries them keeps the fp32-input small tiles under the split arithmetic
    assert _forms(gc.EXPECTED['lstm_side_outputs_chip_filling_split2']) == ['s128']
    assert _forms(gc.EXPECTED['lstm_chip_filling_split2']) == ['s256']
    assert _forms(gc.EXPECTED['lstm_f_side_outputs_split1']) == ['k32']
