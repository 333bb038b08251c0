"""One backward time step of an LSTM layer on the device, per pipeline path, against float64 (C ABI: casv_debug_bwd_step).

Every case of tests/bwd_step_cases.py in both forms -- 0: the fused launch (csrc/gemm_bwd.hip: one, two, three and more unit
groups per K share, the loop up to eight rounds, the atomic and the plain store), 1: lstm_bwd_kernel and the plain GEMM -- through
the two-stage comparator of that module: dz and dc element by element within 4 E_PW of float64, out within the GEMM tests' bounds
of the float64 product of the dz that came back, nothing stored outside the result region (the entry checks the guard rows and
the columns behind N itself; the comparator checks them again on what came back), exact zeros where nothing flows, NaN confined to
the row it entered by.  The statistic shows that the fused launch took the K shares and unit groups the case is in the table for."""
import numpy as np
import pytest

from tests import bwd_step_cases as bs

pytestmark = pytest.mark.gpu

CASES = bs.build_cases()
BOUND = bs.PW_MARGIN * bs.E_PW


@pytest.fixture(scope='module')
def refs():
    """the float64 reference of (case, job): computed once, shared, left unchanged"""
    memo = {}

    def ref(name, j):
        if (name, j) not in memo:
            memo[name, j] = bs.reference(CASES[name].jobs[j])
        return memo[name, j]
    return ref


@pytest.fixture(scope='module')
def engine():
    from cor_asv_ann_amd.engine import HipEngine
    eng = HipEngine(1, 32, 8)
    try:
        yield eng
    finally:
        eng.close()


@pytest.mark.parametrize('name', sorted(CASES))
def test_case_in_every_form_against_float64(engine, refs, name):
    case = CASES[name]
    # (form 1 once more as the "deterministic" step launches it: the plain GEMM without split-K)
    for form, det in [(form, 0) for form in case.forms] + [(1, 1)]:
        engine.set_option('deterministic', det)
        try:
            got = engine.debug_bwd_step(form, case.jobs)
        finally:
            engine.set_option('deterministic', 0)
        shares, groups = engine.stat('bwd_step_shares'), engine.stat('bwd_step_groups')
        assert (shares, groups) == (case.plan[1:] if form == 0 else (0, 0)), (name, form, shares, groups)
        for j, job in enumerate(case.jobs):
            fig, fail = bs.judge(job, refs(name, j), got[j], BOUND)
            print('FIGURES %s form %d%s job %d: %s' % (name, form, ' deterministic' if det else '', j, ' '.join('%s=%.4f' % kv for kv in sorted(fig.items()))))
            assert not fail, (name, form, det, j, fail, fig)


def test_bad_arguments_are_refused_and_leave_the_outputs_untouched(engine):
    """Everything a kernel forms an address from is checked on the host before anything is launched or written."""
    import copy
    from cor_asv_ann_amd._native import NativeError
    good = CASES['top_c1_w64'].jobs[0]
    other = CASES['g1_w96'].jobs[0]

    def outputs(job):
        out = {'dz': np.empty((job.rows + 1, 4 * job.W), np.float32), 'dc': np.empty((job.rows + 1, job.W), np.float32),
               'out': np.empty((job.rows + 1, max(job.ld_out, 1)), np.float32)}
        for v in out.values():
            v.view(np.uint32)[:] = 0x5A5A5A5A
        return out

    def refused(jobs, form=0):
        outs = [outputs(j) for j in jobs]
        with pytest.raises(NativeError) as err:
            engine.debug_bwd_step(form, jobs, outputs=outs)
        assert err.value.code == -1, err.value
        for o in outs:
            for v in o.values():
                assert (v.view(np.uint32) == 0x5A5A5A5A).all()

    def changed(**kw):
        job = copy.copy(good)
        for k, v in kw.items():
            setattr(job, k, v)
        return job
    rows, W = good.rows, good.W
    wide = np.zeros((rows, W + 2), np.float32)
    strided = lambda ld: np.lib.stride_tricks.as_strided(np.zeros(rows * W, np.float32), (rows, W), (4 * ld, 4))
    refused([good], form=2)
    refused([good], form=-1)
    refused([good, good, good])
    refused([good, other])                                       # one width for both jobs
    refused([changed(a=wide[:, :W])])                            # every ld a multiple of 4
    refused([changed(c=wide[:, :W])])
    refused([changed(c_prev=wide[:, 2:])])
    refused([changed(a=strided(W - 4))])                         # ... and at least the width
    refused([changed(c=strided(W - 32))])
    refused([changed(ld_out=good.N - 4)])
    refused([changed(ld_out=good.N + 2)])
    refused([changed(a=None, mask_a=np.ones(W, np.float32))])    # a mask needs its input
    for form in (0, 1):
        refused([good, changed(ld_out=good.N + 1)], form)
    for bad_w in (48, 0, 1056):                                  # W a multiple of 32 in [32, 1024]
        job = bs.Job(4, bad_w, 32)
        job.gates, job.cell, job.dc_in = np.zeros((4, 4 * bad_w), np.float32), np.zeros((4, bad_w), np.float32), np.zeros((4, bad_w), np.float32)
        job.Bt = np.zeros((32, 4 * bad_w), np.float32)
        refused([job])
    engine.debug_bwd_step(0, [good])                             # and the handle still works
