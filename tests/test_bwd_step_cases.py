"""Without a GPU: the case table of tests/bwd_step_cases.py reaches every pipeline of the fused backward step, its restated launch
plan is what csrc/train_plan.h plans (through tests/train_plan_driver.cpp), the float64 reference is autograd's, the float32
restatement passes the comparator with the recorded noise, and every wrong reading of the step is caught on a named case."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import bwd_step_cases as bs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, 'tests', 'train_plan_driver.cpp')

# what the table is built to reach: (blocks, ksplit, gper) per case
PLANS = {
    'g1_w32_n32': (1, 1, 1), 'g1_w32_n96': (2, 1, 1), 'g1_w64': (1, 2, 1), 'g1_w96': (1, 3, 1), 'g1_w160': (6, 5, 1), 'g1_w256': (4, 8, 1),
    'g2_w320': (6, 5, 2), 'g2_plain_store': (161, 1, 2),
    'g3_w288_one_job': (6, 3, 3), 'g3_w288_two_jobs': (9, 3, 3), 'g3_plain_store': (108, 1, 3),
    'g4_w640': (5, 5, 4), 'g5_w800': (14, 5, 5), 'g11_w352': (9, 1, 11), 'two_jobs_uneven': (4, 3, 1),
}
# the case on which each wrong reading must show
WRONG_ON = {
    'mask_per_row': 'g1_w96', 'c_ignored': 'top_c1_w288', 'cprev_from_cell': 'first_step_w288', 'ldb_as_w': 'top_c2_w32',
    'gate_order_ifog': 'g3_w288_one_job', 'dc_in_place': 'g2_w320', 'stage_twice': 'g5_w800', 'stale_last_group': 'g11_w352',
    'rows_past_stored': 'g1_w32_n32',
}


@pytest.fixture(scope='module')
def cases():
    return bs.build_cases()


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    cxx = os.environ.get('CXX') or next((c for c in ('c++', 'g++', 'clang++') if shutil.which(c)), None)
    if not cxx or not shutil.which(cxx):
        pytest.skip('no host compiler')
    exe = str(tmp_path_factory.mktemp('bwd_step_plan') / 'driver')
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', DRIVER, '-o', exe], check=True)
    return exe


def _driver_plans(exe, shapes):
    """[(blocks, ksplit, gper)] of [(W, [(rows, N), ...])] by train_plan.h"""
    lines = []
    for W, jobs in shapes:
        (r0, n0), (r1, n1) = jobs[0], (jobs[1] if len(jobs) > 1 else (0, 0))
        lines.append('B %d %d %d %d %d %d\n' % (len(jobs), W, r0, n0, r1, n1))
    out = subprocess.run([exe], input=''.join(lines), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = [tuple(int(f.split('=')[1]) for f in line.split()[1:]) for line in out.stdout.splitlines()]
    assert len(got) == len(shapes) and all(line.startswith('bwd_step blocks=') for line in out.stdout.splitlines())
    return got


def test_the_plan_equals_the_restatement_on_every_case_and_on_a_sweep(driver, cases):
    shapes = [(c.W, [(j.rows, j.N) for j in c.jobs]) for c in cases.values()]
    assert _driver_plans(driver, shapes) == [c.plan for c in cases.values()]
    for name, want in PLANS.items():
        assert cases[name].plan == want, (name, cases[name].plan)
    # W / 32 in 1..32, 1..400 workgroups, one job and two (the second smaller: the grid is the larger job's)
    sweep = [(32 * g, [(32 * b - 5, 128)] + [(17, 96)] * (count - 1)) for g in range(1, 33) for b in range(1, 401) for count in (1, 2)]
    sweep += [(32 * g, [(33, 128 * b)] * 2) for g in range(1, 33) for b in (1, 2, 3, 53, 54)]
    got = _driver_plans(driver, sweep)
    want = [bs.plan(jobs, W) for W, jobs in sweep]
    assert got == want
    assert {p[0] for p in want} >= set(range(1, 401)) and {p[1] for p in want} == set(range(1, 9))
    # the launcher only runs the plan: no rule of its own
    with open(os.path.join(ROOT, 'cor_asv_ann_amd', 'csrc', 'gemm_bwd.hip')) as f:
        text = f.read()
    launcher = text[text.index('BwdStepPlan launch_lstm_bwd_gemm('):]
    assert 'bwd_step_plan(rows, N, b.count, b.j[0].p.W)' in launcher and 'dim3(plan.blocks, b.count, plan.ksplit)' in launcher
    assert '640' not in launcher and 'ksplit = ' not in launcher


def test_the_table_reaches_every_pipeline_and_input_form(cases):
    fused = [c for c in cases.values() if 0 in c.forms]
    gper = {c.plan[2] for c in fused}
    assert {1, 2, 3, 4, 5} <= gper and max(gper) >= 6
    plain = {c.plan[2] for c in fused if c.plan[1] == 1}                 # the store that is no atomic
    assert {1, 2, 3} <= plain and max(plain) >= 6
    assert {c.plan[1] for c in fused} >= {1, 2, 3, 5, 8}
    looped = [c for c in fused if c.plan[2] >= 3]

    def reached(pred):
        return any(pred(j) for c in fused if c.plan[2] == 1 for j in c.jobs) and any(pred(j) for c in looped for j in c.jobs)
    ld = lambda x: x.strides[0] // 4
    assert reached(lambda j: j.a is not None and j.mask_a is not None and j.b is not None and j.c_prev is not None)
    assert reached(lambda j: j.b is None and j.a is not None and j.mask_a is not None)                      # the last step
    assert reached(lambda j: j.c_prev is None)                                                             # the first step
    assert reached(lambda j: j.a is None)
    assert reached(lambda j: j.a is not None and ld(j.a) == 2 * j.W)
    for ctx in (1, 2):                                                                                     # the top cell, C = W and C = 2W
        assert reached(lambda j: j.N == j.ld_out == (ctx + 1) * j.W and j.b is not None and ld(j.b) == j.N and j.c is not None and j.mask_a is None)
    assert reached(lambda j: j.N == 2 * j.W and j.b is None and j.c is None and j.mask_a is None and j.a is not None)
    assert reached(lambda j: j.ld_out > j.N) and reached(lambda j: j.c_prev is not None and ld(j.c_prev) > j.W)
    assert reached(lambda j: j.mask_a is not None and (j.mask_a == 0).any())
    assert reached(lambda j: (j.gates == 0).any() and (j.gates == 1).any())
    assert reached(lambda j: (np.abs(np.tanh(j.cell)) == 1).any())
    assert reached(lambda j: bool(j.nan_rows))
    assert {c.jobs[0].rows for c in fused} >= {1, 5, 31, 32, 33, 65}
    two = cases['two_jobs_uneven'].jobs
    assert [(j.rows, j.N) for j in two] == [(5, 96), (37, 160)]
    gs = cases['grid_stride']
    assert gs.forms == (1,) and gs.jobs[0].rows * gs.W > 4096 * 256
    assert set(WRONG_ON) == set(bs.WRONG) and set(WRONG_ON.values()) <= set(cases)


def test_the_restatement_passes_and_the_recorded_noise_is_what_it_measures(cases):
    e_pw = 0.0
    for case in cases.values():
        for j, job in enumerate(case.jobs):
            fig, fail = bs.judge(job, bs.reference(job), bs.restate(job), bs.E_PW)
            assert not fail, (case.name, j, fail)
            e_pw = max(e_pw, fig['pw'])
    assert 0 <= bs.E_PW - e_pw < 1e-3, e_pw          # (recorded rounded up to three decimals)
    with open(os.path.join(ROOT, 'profiles', 'bwd_step_noise.txt')) as f:
        assert 'E_PW = %.3f' % bs.E_PW in f.read()


@pytest.mark.parametrize('wrong', bs.WRONG)
def test_every_wrong_reading_is_caught(cases, wrong):
    """by >= 10 x the device's bound, or by an exact check"""
    case = cases[WRONG_ON[wrong]]
    bound = bs.PW_MARGIN * bs.E_PW
    caught = False
    for job in case.jobs:
        ref = bs.reference(job)
        fig, fail = bs.judge(job, ref, bs.restate(job, wrong), bound)
        exact = [f for f in fail if 'units' not in f]
        by_ten = fig.get('pw', 0) >= 10 * bound or fig.get('max', 0) >= 10 * bs.MAX_BOUND or fig.get('rms', 0) >= 10 * bs.RMS_BOUND
        assert not fail or exact or by_ten, (wrong, fail, fig)          # (a miss by less than 10 x would be luck)
        caught = caught or bool(exact) or by_ten
    assert caught, wrong


def test_a_stage_counted_twice_is_a_thousand_units(cases):
    job = cases['g5_w800'].jobs[0]
    fig, fail = bs.judge(job, bs.reference(job), bs.restate(job, 'stage_twice'), bs.PW_MARGIN * bs.E_PW)
    assert fig['pw'] <= bs.E_PW and fig['max'] >= 1e3, fig          # the pointwise stage is clean: only the contraction shows it


@pytest.mark.parametrize('first', [False, True])
def test_the_reference_is_autograd_through_one_step(first):
    """h = o tanh(c), c = f c_prev + i g with the gates' activations of pre-activations z: d(sum(h dh) + sum(c dc_in)) / dz and
    / dc_prev by torch autograd in float64 equal the reference's dz and dc to 1e-12."""
    import torch
    rows, W = 7, 64
    rng = np.random.default_rng(5 + first)
    z = torch.tensor(rng.standard_normal((4, rows, W)), dtype=torch.float64, requires_grad=True)
    cp = torch.tensor(np.zeros((rows, W)) if first else rng.standard_normal((rows, W)), dtype=torch.float64, requires_grad=True)
    i, f, o = torch.sigmoid(z[0]), torch.sigmoid(z[1]), torch.sigmoid(z[3])
    g = torch.tanh(z[2])
    c = f * cp + i * g
    h = o * torch.tanh(c)
    job = bs.Job(rows, W, W)
    job.a, job.mask_a = rng.standard_normal((rows, W)), (rng.random(W) >= 0.25) / 0.75
    job.b = None if first else rng.standard_normal((rows, W))
    job.c = rng.standard_normal((rows, W))
    job.c_prev = None if first else cp.detach().numpy()
    job.dc_in = rng.standard_normal((rows, W))
    job.gates = bs._join([x.detach().numpy() for x in (i, f, g, o)])
    job.cell = c.detach().numpy()
    dh = job.a * job.mask_a + (0 if first else job.b) + job.c
    ((h * torch.tensor(dh)).sum() + (c * torch.tensor(job.dc_in)).sum()).backward()
    ref = bs.reference(job)
    assert np.abs(ref['dz'] - bs._join([z.grad[k].numpy() for k in range(4)])).max() < 1e-12
    assert np.abs(ref['dc'] - cp.grad.numpy()).max() < 1e-12
