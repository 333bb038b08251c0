"""The operand machinery of the fused LSTM GEMM, form by form, against float64 (C ABI: casv_debug_gemm_jobs -> launch_gemm_batch).

Everything of csrc/gemm_args.h that a plain C = A . B^T never uses -- K segments with koff and ld != width, gathered rows, step
addressing by immediate and by device word, the step-0 forms, the cell state, live rows, ragged M, mixed batches -- on the cases of
tests/lstm_gemm_cases.py, in each launch form that can take them: 128x128, 32x128 and 64x128 tiles on the fp32-input instruction,
128x128 and 256x256 tiles on split operands (the latter with a pre-split weight image and with staging).  Per case: the statistic
shows the intended form; every live output passes the comparator against float64 (bounds derived in lstm_gemm_cases.py from the
project's own: no number is invented here); the fp32-input forms agree bit for bit, and so do the two split tile shapes; every byte
the launch must not store to is still 0xFF (the guard row behind each output is checked by the entry itself)."""
import time

import numpy as np
import pytest

from tests import lstm_gemm_cases as lg

pytestmark = pytest.mark.gpu

SMALL = ['a_bias', 'a_nobias', 'b_step_plus', 'b_step_minus', 'c_skip_first', 'c_first_base', 'd_two_jobs', 'd_plain_rider', 'd_four_jobs',
         'e_straddle_dead', 'e_straddle_live', 'e_finished_lines', 'f_side_outputs', 'p_plain_launch']
BIG = ['s_8448', 's_8492', 's_8192_lines_of_8', 's_8448_lines_of_8', 's_first_base', 's_step']
UNTOUCHED = np.uint32(0xFFFFFFFF)
# rows no tile shape may store to: no tile that holds them has a live row
DEAD_BLOCKS = {'e_straddle_dead': [(128, 256)], 'e_finished_lines': [(256, 512), (768, 1024)],
               's_8192_lines_of_8': [(512, 768)], 's_8448_lines_of_8': [(512, 768), (8192, 8320)]}


@pytest.fixture(scope='module')
def cases():
    return lg.build_cases()


@pytest.fixture(scope='module')
def refs(cases):
    """the float64 reference of (case, job, step): computed once, shared, left unchanged.  (Those of the chip-filling cases are
    hundreds of MB each and serve one test: that test drops them.)"""
    memo = {}

    def ref(name, j, step):
        if (name, j, step) not in memo:
            memo[name, j, step] = lg.reference(cases[name], cases[name].jobs[j], step)
        return memo[name, j, step]
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


def test_the_lists_name_every_case(cases):
    assert sorted(SMALL + BIG) == sorted(cases) and set(DEAD_BLOCKS) <= set(cases)


def _launch(eng, case, form, step, by_ptr=False):
    """The case under the options of `form`: per job {name: (slots, M, ld)}.  The statistic must show the intended form."""
    opt = lg.OPTIONS[form]
    eng.set_option('tile', opt['tile'])
    eng.set_option('split_bf16', opt['split_bf16'])
    for job in case.jobs:
        job.b_static = form == 'split2_image'
    outs, forms, launches = eng.debug_gemm_jobs(case.epi, case.jobs, step, by_ptr)
    want = lg.intended_forms(case, form)
    if forms != lg.form_mask(want) and eng.stat('cus') != 256:
        pytest.skip('this device has %d CUs, not 256: %s under %s plans to the forms %#x, the case is meant for %s'
                    % (eng.stat('cus'), case.name, form, forms, '+'.join(want)))
    assert forms == lg.form_mask(want) and launches == len(want), (case.name, form, forms, launches)
    return outs


def _addressed(case, job, out, step, live):
    """{name: (M, width)} of the slots the step selects; every other slot, every column behind the width and the rows of DEAD_BLOCKS
    must be untouched, and no element of a live row may be left unwritten"""
    lstm = case.lstm(job)
    widths = {'out': job.N // 4 if lstm else job.N, 'c_out': job.N // 4, 'gates_out': job.N, 'out2': job.N // 4}
    res = {}
    for name, full in out.items():
        slots, ld, mul, add = getattr(job, name)
        slot, width, bits = step * mul + add, widths[name], full.view(np.uint32)
        assert (bits[np.arange(slots) != slot] == UNTOUCHED).all(), (case.name, name, 'a store into another slot')
        assert (bits[slot][:, width:] == UNTOUCHED).all(), (case.name, name, 'a store behind the row')
        assert not (bits[slot][live, :width] == UNTOUCHED).any(), (case.name, name, 'a live element was not written')
        for lo, hi in DEAD_BLOCKS.get(case.name, []):
            assert (bits[slot][lo:hi] == UNTOUCHED).all(), (case.name, name, 'a tile without a live row was stored', lo, hi)
        res[name] = full[slot][:, :width]
    return res


def _run_forms(eng, case, refs, step, forms):
    """{form: [per job {name: (M, width)}]}, every job judged against float64"""
    got = {}
    for form in forms:
        t0 = time.perf_counter()
        outs = _launch(eng, case, form, step)
        call = time.perf_counter() - t0
        got[form] = []
        for j, job in enumerate(case.jobs):
            ref = refs(case.name, j, step)
            res = _addressed(case, job, outs[j], step, ref.live)
            fig, ok = lg.judge(case, job, ref, res)
            print('FIGURES %s step %d job %d %s: %s (call %.2f s)' % (case.name, step, j, form, ' '.join('%s=%.4f' % kv for kv in sorted(fig.items())), call))
            assert ok, (case.name, step, j, form, fig)
            if 'out2' in res:
                assert np.array_equal(res['out2'][ref.live].view(np.uint32), res['out'][ref.live].view(np.uint32)), (case.name, form)
            got[form].append(res)
    return got


def _same_bits(case, refs, step, got, forms):
    """the live rows of every output agree bit for bit between `forms`"""
    forms = [f for f in forms if f in got]
    for form in forms[1:]:
        for j in range(len(case.jobs)):
            live = refs(case.name, j, step).live
            for name, first in got[forms[0]][j].items():
                same = np.array_equal(first[live].view(np.uint32), got[form][j][name][live].view(np.uint32))
                assert same, (case.name, step, j, name, '%s and %s differ in bits' % (forms[0], form))


@pytest.mark.parametrize('name', SMALL)
def test_small_case_in_every_form(engine, cases, refs, name):
    case = cases[name]
    for step in case.steps:
        got = _run_forms(engine, case, refs, step, case.forms)
        _same_bits(case, refs, step, got, lg.FP32_FORMS)
        _same_bits(case, refs, step, got, lg.SPLIT_FORMS)       # (mode 2 of a launch too small for 256x256 tiles: 128x128 split tiles)


@pytest.mark.parametrize('name', ['b_step_plus', 'b_step_minus', 's_step'])
def test_the_step_through_a_device_word_gives_the_bits_of_the_immediate_step(engine, cases, name):
    case = cases[name]
    for form in case.forms:
        imm = _launch(engine, case, form, case.steps[0])
        ptr = _launch(engine, case, form, case.steps[0], by_ptr=True)
        for a, b in zip(imm, ptr):
            for key in a:
                assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), (name, form, key)


@pytest.mark.parametrize('name,step', [(name, step) for name in BIG for step in ((3,) if name == 's_step' else (0, 3))])
def test_chip_filling_case_on_both_split_tile_shapes(engine, cases, refs, name, step):
    """N = 2048, Ktot = 160: whole rounds as 256x256 tiles, with the weight as a pre-split image and staged; the partial round and a
    ragged last block behind the cut as 128x128 split tiles.  Mode 2 equals mode 1 bit for bit."""
    case = cases[name]
    try:
        got = _run_forms(engine, case, refs, step, case.forms)
        _same_bits(case, refs, step, got, lg.SPLIT_FORMS)
    finally:
        refs.drop(name)


def test_bad_arguments_are_refused_before_anything_is_launched(engine, cases):
    """Everything a kernel forms an address from is checked on the host: these tests can never be a way to read or write outside a
    buffer.  Each of these descriptions is refused with CASV_ERR_ARG."""
    import copy
    from cor_asv_ann_amd._native import NativeError
    case = cases['a_bias']

    def refused(step=2, by_ptr=False, epi=1, **change):
        job = copy.copy(case.jobs[0])
        job.segs = [copy.copy(s) for s in job.segs]
        job.c_in = copy.copy(job.c_in)
        for key, value in change.items():
            target, _, field = key.rpartition('__')
            obj = job if not target else job.c_in if target == 'c_in' else job.segs[int(target[3:])]
            setattr(obj, field, value)
        with pytest.raises(NativeError) as err:
            engine.debug_gemm_jobs(epi, [job], step, by_ptr)
        assert err.value.code == -1, (change, err.value)
    job = case.jobs[0]
    rows = job.segs[0].rows.copy()
    rows[299] = job.segs[0].pool.shape[1]
    refused(seg0__rows=rows)                                    # an index past the pool
    rows[299] = -1
    refused(seg0__rows=rows)
    refused(c_in__rows=rows)
    refused(seg2__pool=job.segs[2].pool[:, :299])               # ungathered rows need M pool rows
    refused(step=3)                                             # the slot lies outside the pools
    refused(seg1__step_add=-3)
    refused(out=(2, 96, 1, 0))                                  # ... outside the output
    refused(c_out=(4, 68, 1, 2))
    refused(seg0__width=48)                                     # widths are multiples of 32
    refused(seg1__width=128)                                    # ld >= width
    refused(seg0__koff=112)                                     # koff + width <= Ktot
    refused(seg0__koff=98)
    refused(Ktot=96, Bt=job.Bt[:, :96])                         # the widths' sum <= Ktot
    refused(N=192, Bt=job.Bt[:192], bias=job.bias[:192])        # N % 128 for the cell
    refused(out=(4, 60, 1, 0))                                  # ld >= the output's width, a multiple of 4
    refused(out=(4, 98, 1, 0))
    refused(nact=np.full(4, 100, np.int32), nact_group=128)     # one entry per line, at most nact_group live rows
    refused(nact=np.full(2, 100, np.int32), nact_group=128)
    refused(nact=np.full(3, 129, np.int32), nact_group=128)
    refused(gates_out=(4, 288, 1, 0), epi=0)                    # side outputs belong to the cell
    refused(step=2, by_ptr=True, seg0__step_add=-1)             # through the device word the job must be valid at step 0 too
    ok = cases['b_step_plus']
    engine.debug_gemm_jobs(1, ok.jobs, 3, True)
