"""Without a GPU: the case table of tests/train_form_cases.py reaches every instantiation the train step's dispatchers name, its
restated form decision (train_form) is what csrc/train_plan.h decides, the noise bounds would see a persistent kernel that gets a
row-block edge or a job's last step wrong, and no case measures against a degenerate noise unit.

The plan is held by behaviour: a stand-alone driver (tests/train_plan_driver.cpp: train_plan.h and the standard library, built
with the host compiler, -Wall -Werror, and once more under the address and undefined-behaviour sanitizers) plans what train_form
plans, and every record must be equal.  Which means holds which fact of the form:
  row block 32, workgroups per CU 2 / 2 / 1 / 1, counters 2 / 16 / 3 / 12, cap 16 as one constant, 64 CUs, T <= 288
        the driver's constants (test_the_constants_and_the_widths_with_a_form); their effect, by the records of every case on six
        CU counts and six residency figures (test_the_plan_equals_the_restatement_...: grids, counter bytes, the capped sites of
        depth 8, nothing below 64 CUs); the kernel files' own row blocks by their static_assert against the header's
  the four shape conditions and their labels
        the sweep of test_the_constants_and_the_widths_with_a_form: which NT have a form per kind, beside multiples of 32, at W != C,
        C = 1056, no rows, no steps, 0 and 3 jobs -- equal to train_form_cases.grid and NT
  the same labels in the grid and in the launcher
        there is one list per kind (the driver prints it); that every instantiation comes from it is structure:
        test_the_plan_is_pure_and_the_sources_only_run_it, and tests/test_gpu_train_forms.py runs every one of them
  one deciding place and one counting place, used by exactly four sites
        the plan counts (the records' slots and the step's count); that train.hip asks it in one function, called by the four
        sites and by nothing else, and never counts itself is structure (same test)
  one slot size, the maximum, for addresses, allocation and clear
        the records' offsets and slot_bytes (equal to the largest kind's counters); that allocation and clear use the same function
        is structure (same test)
  the cell's, the backward's and the split's own conditions, the defer rule
        test_the_site_conditions_each_decide: each flag off, T = 288 / 289, W = 96, CASV_ATTN_DEFER 0 / 1 / 3
  the gate (option, deterministic, back-off)
        every case under each of them (test_the_plan_equals_the_restatement_...)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import grad_noise_cases as gn
from tests import train_form_cases as tf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'cor_asv_ann_amd', 'csrc')


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _function(text, head):
    """The body of the function whose definition starts with `head` (up to the first line that is a lone closing brace)."""
    i = text.index(head)
    return text[i:text.index('\n}', i)]


# ------------------------------------------------------------------------------------------------------------------ 1. reachability
def test_table_reaches_every_instantiation_and_form():
    reached = {k: set() for k in tf.NT}
    split_nt, jobs, unequal, counts = set(), set(), set(), set()
    for fc in tf.ALL:
        f = tf.form(fc)
        assert f['count'] == fc[2], (fc[0][0], f['count'])          # the table states every case's predicted count
        counts.add(f['count'])
        for ln in f['launches']:
            if not ln['persistent']:
                continue
            reached[ln['kind']].add(ln['NT'])
            if ln['split']:
                split_nt.add(ln['NT'])
            if ln['kind'] in ('rec', 'rec_bwd'):
                jobs.add((ln['kind'], ln['jobs']))
                if ln['jobs'] == 2 and ln['lengths'][0] != ln['lengths'][1]:
                    T, U = (ln['lengths'] if ln['kind'] == 'rec' else ln['lengths'][::-1])
                    unequal.add((ln['kind'], 'T>U' if T > U else 'T<U'))
    # every dispatcher label, listed
    assert sorted(reached['rec']) == list(range(1, 17))
    assert sorted(reached['rec_bwd']) == [4, 8, 12, 16]
    assert sorted(reached['cell']) == [4, 8, 16]
    assert sorted(reached['cell_bwd']) == [4, 8, 16] and sorted(split_nt) == [4, 8, 16]
    assert {k: tuple(sorted(v)) for k, v in reached.items()} == tf.NT
    assert jobs == {('rec', 1), ('rec', 2), ('rec_bwd', 1), ('rec_bwd', 2)}
    assert unequal == {(k, s) for k in ('rec', 'rec_bwd') for s in ('T>U', 'T<U')}
    assert tf.CAP in counts and 0 in counts


def test_depth_8_reaches_the_cap_and_names_what_falls_back():
    f = tf.form(tf.BY_NAME['d8_plain'])
    assert f['count'] == tf.CAP == 16 and f['capped'] == tf.DEPTH8_CAPPED
    assert [ln['layers'] for ln in f['launches'] if ln['capped']] == tf.DEPTH8_CAPPED
    assert all(ln['persistent'] for ln in f['launches'][:16]) and len(f['launches']) == 18


def test_residency_edge_and_the_stepwise_path():
    assert tf.form(tf.BY_NAME['w256_b1024'])['count'] == 6 and tf.form(tf.BY_NAME['w256_b1025'])['count'] == 0
    f = tf.form(tf.BY_NAME['w256_b1024'])
    assert [ln['grid'] for ln in f['launches']] == [512, 512, 256, 256, 512, 512]
    assert tf.form(tf.BY_NAME['w256_b1025'], cus=264)['count'] == 6         # (one more row block: a device of 264 CUs would hold it)
    assert all(tf.form(fc, persistent=False)['count'] == 0 for fc in tf.ALL)
    assert all(tf.form(fc, cus=63)['count'] == 0 for fc in tf.ALL)


def test_every_case_has_ragged_sources_and_targets_where_its_shape_allows():
    for fc in tf.ALL:
        (name, d, W, V, B, L, es, mk, flags, A, frozen), S, _ = fc
        cfg, w, (enc_in, dec_in, dec_out, wts, masks), batch = tf.build(fc)
        sidx = batch[0] if A == 1 else batch[0][:, :, 0]
        T = S + 1
        assert sidx.shape == (B, T) and batch[2].shape == (B, L + 2), name
        lens = (sidx >= 0).sum(axis=1)
        assert ((sidx >= 0) == (np.arange(T)[None, :] < lens[:, None])).all() and lens.max() == T and lens.min() >= 1
        assert (sidx[np.arange(B), lens - 1] == 1).all()                # (every line ends in the end character)
        assert (enc_in[sidx < 0] == 0).all() and (masks is not None) == mk
        if B >= 3:
            assert lens.min() == min(2, S) and 0.2 <= (lens < T).mean() <= 0.4, (name, lens)
        if B >= 2 and L >= 2:
            assert (np.asarray(wts) > 0).sum(axis=1).min() < L + 1, name


# ------------------------------------------------------------------------------------------------------------------ 2. the restatement
DRIVER = os.path.join(ROOT, 'tests', 'train_plan_driver.cpp')
CUS = (256, 304, 264, 128, 64, 63)              # the MI355X, larger parts (264: one more row block fits), smaller ones, one below MIN_CUS
PER_CU = ((2, 2, 1, 1), (1, 1, 1, 1), (0, 2, 1, 1), (2, 0, 1, 1), (2, 2, 0, 1), (2, 2, 1, 0))     # as planned for, one each, a failed query per kind
GATES = (dict(), dict(deterministic=True), dict(backoff=True))


def _cxx():
    cxx = os.environ.get('CXX') or next((c for c in ('c++', 'g++', 'clang++') if shutil.which(c)), None)
    if not cxx or not shutil.which(cxx):
        pytest.skip('no host compiler')
    return cxx


def _site_condition_steps():
    """[(key, train_form)] beside the table: every site condition with its flag off, the switches' values, the defer rule's edges."""
    from oracle import ModelConfig
    cfg = ModelConfig(depth=2, width=128, voc_size=40)
    out = [('all_on', tf.train_form(cfg, 33, 5, 11))]
    out += [('kr_off', tf.train_form(cfg, 33, 5, 11, not_plain=('rec_bwd',))), ('hs_ld_off', tf.train_form(cfg, 33, 5, 11, not_plain=('cell',)))]
    out += [('split_opt_off', tf.train_form(cfg, 33, 5, 11, split=False)), ('split_gave_up', tf.train_form(cfg, 33, 5, 11, split_off=True)),
            ('rows_do_not_fit', tf.train_form(cfg, 33, 5, 11, rows_fit=False))]
    out += [('defer%d_t%d' % (d, T), tf.train_form(cfg, 33, T, 11, defer=d)) for d in (0, 1, 3) for T in (288, 289)]
    out += [('defer%d_w96' % d, tf.train_form(ModelConfig(depth=2, width=96, voc_size=40), 33, 5, 11, defer=d)) for d in (1, 3)]
    return out


def _steps():
    """[(key, train_form)] of every case of the table on every CU count, option value and residency, under every gate."""
    out = []
    for gate in GATES:
        for fc in tf.ALL:
            for cus in CUS:
                for on in (True, False):
                    for per_cu in PER_CU:
                        key = '%s|%d|%d|%s|%s' % (fc[0][0], cus, on, '%d%d%d%d' % per_cu, ''.join(gate))
                        out.append((key, tf.form(fc, cus=cus, persistent=on, blocks_per_cu=per_cu, **gate)))
    return out + _site_condition_steps()


def _run(exe, lines):
    out = subprocess.run([exe], input=''.join(line + '\n' for line in lines), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.splitlines()


def _plan_steps(exe, steps):
    """The driver's records of the steps, per step: the sites' records and the step's count."""
    got = _run(exe, [line for key, f in steps for line in tf.driver_lines(key, f)])
    out, at = [], 0
    for key, f in steps:
        n = len(f['launches']) + 2
        assert got[at] == 'case ' + key
        out.append(got[at + 1:at + n])
        at += n
    assert at == len(got)
    return out


@pytest.fixture(scope='module')
def steps():
    return _steps()


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('train_plan') / 'driver')
    subprocess.run([_cxx(), '-std=c++17', '-O1', '-Wall', '-Werror', DRIVER, '-o', exe], check=True)
    return exe


def test_the_plan_equals_the_restatement_on_every_case_cu_count_and_gate(driver, steps):
    """train_plan.h (through tests/train_plan_driver.cpp) against train_form: every site's record -- persistent, capped, grid, NT, slot,
    slot offset, the kind's counter bytes, defer, split -- and every step's count and slot size, in sites()'s order."""
    assert len(set(k for k, _ in steps)) == len(steps) == len(GATES) * len(tf.ALL) * len(CUS) * 2 * len(PER_CU) + 14
    got = _plan_steps(driver, steps)
    wrong = [(k, g, tf.records(f)) for (k, f), g in zip(steps, got) if g != tf.records(f)]
    assert not wrong, 'first of %d: %r' % (len(wrong), wrong[0])
    by_key = {k: f for k, f in steps}
    # the inputs decide: the gate's four, the CU count and the residency figure each change a count
    plain = '|256|1|2211|'
    assert by_key['w256_b1024' + plain]['count'] == 6 and by_key['w256_b1025' + plain]['count'] == 0
    assert by_key['w256_b1025|264|1|2211|']['count'] == 6 and by_key['w256_b1024|256|1|1111|']['count'] == 2
    assert by_key['w128_b33|256|1|0211|']['count'] == 4 and by_key['w128_b33|256|1|2210|']['count'] == 5
    assert all(f['count'] == 0 for k, f in steps if '|63|' in k or re.search(r'\|0\|\d{4}\|', k) or 'deterministic' in k or 'backoff' in k)
    assert all(f['count'] == fc[2] for fc in tf.ALL for f in [by_key[fc[0][0] + plain]])
    # the slots: one size per step, the backward recurrence's counters; consecutive; the give-up word behind the kind's own counters
    f = by_key['d8_plain' + plain]
    assert f['slot_bytes'] == tf.counter_bytes('rec_bwd', 5) == (16 * 32 + 32) * 4
    assert [ln['offset'] for ln in f['launches']] == [i * f['slot_bytes'] for i in range(16)] + [0, 0]
    assert {ln['kind']: ln['counters'] for ln in f['launches'] if ln['persistent']} == {k: (tf.COUNTERS[k] * 32 + 32) * 4 for k in tf.KINDS}
    assert by_key['w128_b33' + plain]['slot_bytes'] == (2 * 16 * 32 + 32) * 4


def test_the_site_conditions_each_decide(driver):
    """The sites' own conditions, each with its flag off: one job's kr != W, hs_ld != W, the split's three inputs, the defer rule."""
    steps = _site_condition_steps()
    got = _plan_steps(driver, steps)
    assert [tf.records(f) for _, f in steps] == got
    f = dict(steps)
    kinds = lambda name: [(ln['kind'], ln['persistent']) for ln in f[name]['launches']]
    assert f['all_on']['count'] == 6 and kinds('all_on') == [(k, True) for k in ('rec', 'rec', 'cell', 'cell_bwd', 'rec_bwd', 'rec_bwd')]
    assert f['kr_off']['count'] == 4 and [k for k, on in kinds('kr_off') if not on] == ['rec_bwd', 'rec_bwd']
    assert f['hs_ld_off']['count'] == 5 and [k for k, on in kinds('hs_ld_off') if not on] == ['cell']
    cell_bwd = lambda name: [ln for ln in f[name]['launches'] if ln['kind'] == 'cell_bwd'][0]
    assert cell_bwd('all_on')['split'] and (cell_bwd('all_on')['defer'], cell_bwd('all_on')['slot']) == (1, 3)
    for name in ('split_opt_off', 'split_gave_up', 'rows_do_not_fit'):
        assert f[name]['count'] == 6 and not cell_bwd(name)['split'] and cell_bwd(name)['persistent'], name
    assert [cell_bwd('defer%d_t%d' % (d, T))['defer'] for d in (0, 1, 3) for T in (288, 289)] == [0, 0, 1, 0, 3, 0]
    assert all(cell_bwd('defer%d_t289' % d)['persistent'] and cell_bwd('defer%d_t289' % d)['split'] for d in (0, 1, 3))
    assert not cell_bwd('defer3_w96')['persistent'] and cell_bwd('defer3_w96')['defer'] == 0 and f['defer3_w96']['count'] == 2


def test_the_constants_and_the_widths_with_a_form(driver):
    """The header's numbers, and which NT have a form: every kind at W = 32 ... 640, beside multiples of 32, at W != C and C = 1056."""
    got = _run(driver, ['K'])
    assert got[0] == 'constants row_block=%d cap=%d min_cus=%d defer_max_t=%d' % (tf.ROW_BLOCK, tf.CAP, tf.MIN_CUS, tf.DEFER_MAX_T)
    assert (tf.ROW_BLOCK, tf.CAP, tf.MIN_CUS, tf.DEFER_MAX_T) == (32, 16, 64, 288)
    assert got[1:] == ['kind %s per_cu=%d counters=%d widths=%s' % (k, tf.BLOCKS_PER_CU[k], tf.COUNTERS[k], ''.join('%d,' % n for n in tf.NT[k]))
                       for k in tf.KINDS]
    assert [(tf.BLOCKS_PER_CU[k], tf.COUNTERS[k]) for k in tf.KINDS] == [(2, 2), (2, 16), (1, 3), (1, 12)]
    shapes = [(W, W) for W in range(32, 641, 32)] + [(136, 136), (100, 100), (128, 256), (256, 128), (1056, 1056)]
    rows = [(k, W, C, 33, 3, jobs) for k in tf.KINDS for W, C in shapes for jobs in (1, 2)]
    rows += [(k, 128, 128, B, U, jobs) for k in tf.KINDS for B, U, jobs in ((0, 3, 1), (1, 0, 1), (1, 3, 0), (1, 3, 3))]
    got = _run(driver, ['G %s %d %d %d %d %d 256 %d' % (r + (tf.BLOCKS_PER_CU[r[0]],)) for r in rows])
    assert got == ['grid=%d' % tf.grid(k, W, C, B, jobs, 256, tf.BLOCKS_PER_CU[k], U) for k, W, C, B, U, jobs in rows]
    have = {k: tuple(sorted({W // 32 for (kk, W, C, *_), g in zip(rows, got) if kk == k and g != 'grid=0'})) for k in tf.KINDS}
    assert have == tf.NT
    grid_of = {r: int(g[5:]) for r, g in zip(rows, got)}
    assert grid_of[('rec', 128, 256, 33, 3, 2)] == 16 and grid_of[('rec_bwd', 128, 256, 33, 3, 2)] == 16      # (the recurrences do not look at C)
    assert grid_of[('cell', 128, 256, 33, 3, 1)] == grid_of[('cell_bwd', 256, 128, 33, 3, 1)] == 0 and grid_of[('cell', 128, 128, 33, 3, 2)] == 8
    assert all(grid_of[(k, 128, 128, 0, 3, 1)] == 0 for k in tf.KINDS)
    assert [grid_of[(k, 128, 128, 1, 0, 1)] for k in tf.KINDS] == [4, 4, 0, 0]
    assert [grid_of[(k, 128, 128, 1, 3, j)] for k in tf.KINDS for j in (0, 3)] == [0, 0, 0, 0, 4, 4, 4, 4]


def test_the_driver_is_clean_under_the_host_sanitizers(tmp_path, driver, steps):
    cxx = _cxx()
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    flags = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer']
    if subprocess.run([cxx] + flags + [str(probe), '-o', str(tmp_path / 'probe')], capture_output=True).returncode != 0:
        pytest.skip('the host compiler has no sanitizer runtime')
    exe = str(tmp_path / 'driver_san')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Werror'] + flags + [DRIVER, '-o', exe], check=True)
    lines = ['K'] + [line for key, f in steps for line in tf.driver_lines(key, f)]
    assert _run(exe, lines) == _run(driver, lines)


def _code(text):
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', text, flags=re.S))


def test_the_plan_is_pure_and_the_sources_only_run_it():
    """What behaviour cannot show: train_plan.h knows no device and no environment; every instantiation of the five kernels comes
    from its lists; train.hip asks it in one place, which the four sites call; one slot size serves addresses, allocation and clear."""
    plan = _src('train_plan.h')
    assert not re.search(r'\bhip|getenv', _code(plan), re.I)
    assert re.findall(r'#include [<"]([^>"]+)[>"]', plan) == ['algorithm', 'cstddef']
    assert re.findall(r'#include [<"]([^>"]+)[>"]', open(DRIVER).read())[0] == '../cor_asv_ann_amd/csrc/train_plan.h'
    files = {'train_persist.hip': ('REC', [tf.KERNEL['rec']]), 'train_persist_bwd.hip': ('REC_BWD', [tf.KERNEL['rec_bwd']]),
             'train_persist_top.hip': ('CELL', [tf.KERNEL['cell']]), 'train_persist_topb.hip': ('CELL_BWD', [tf.KERNEL['cell_bwd'], tf.SPLIT_KERNEL])}
    csrc = {n: _code(_src(n)) for n in os.listdir(CSRC) if n.endswith(('.hip', '.h'))}
    # the row block and the stage are train_tile.h's alone: one static_assert there, and the four files define no such constant
    assert csrc['train_tile.h'].count('static_assert(BM == TRAIN_ROW_BLOCK') == 1
    assert sum(code.count('== TRAIN_ROW_BLOCK') for code in csrc.values()) == 1
    for name, (widths, kernels) in files.items():
        code = csrc[name]
        assert '#include "train_tile.h"' in code, name
        assert not re.search(r'constexpr int \w*(BM|BN|K2|LD|STAGE)\b', code), name
        assert 'switch (train_width_nt(' in code and not re.search(r'case \d+:', code), name           # (no hand-written width switch)
        for kernel in kernels:
            # a width's instantiation is named in ONE place, a case generated from the kind's list; elsewhere only as a template of NT
            uses = re.findall(r'%s<(\w+)>' % kernel, code)
            assert sorted(set(uses)) == ['NT', 'NT_'] or uses == ['NT_'], (kernel, uses)
            assert uses.count('NT_') == 1, (kernel, uses)
            line = [ln for ln in code.splitlines() if kernel + '<NT_>' in ln][0]
            macro = re.match(r'#define (\w+)\(NT_\) case NT_: return ', line).group(1)
            assert code.count('CASV_TRAIN_%s_WIDTHS(%s)' % (widths, macro)) == 1, kernel
            assert all(kernel + '<' not in other for n, other in csrc.items() if n != name), kernel
        assert 'TRAIN_BLOCKS_PER_CU[TRAIN_%s]' % widths in code and not re.search(r'persist_blocks_per_cu\([^;]*, \d+\)', code), name
    train = _code(_src('train.hip'))
    # one asking place, called by exactly the four sites; nothing else in the sources plans, counts or sizes
    assert train.count('.next(') == 1 and '.next(gate, site)' in _function(train, 'static int persist_launch(')
    callers = [name for head, name in re.findall(r'^((?:static )?\w+ (\w+)\()', train, re.M)      # (the phases scoring shares are not static: train_step.h)
               if name != 'persist_launch' and 'persist_launch(' in _function(train, head)]
    assert sorted(callers) == ['cell_backward_persistent', 'forward_cell', 'layers_backward', 'layers_forward']
    assert train.count('persist_launch(m, ') == 4 and train.count('PC_PERSIST') == 2 and train.count('persist_give_up_word(') == 1
    assert not re.search(r'plan\.launches\s*(\+\+|--|[-+]?=[^=])|(\+\+|--)\s*\w*(->|\.)?plan\.launches', train)      # (only the plan counts)
    assert 'ts->plan = TrainStepPlan{}' in _function(train, '\nint stage_inputs(Step& s) {')
    assert train.count('train_slot_bytes(') == 2 and train.count('slot_offset') == 1
    assert 'TRAIN_LAUNCH_CAP * train_slot_bytes(B)' in _function(train, '\nint plan_buffers(Step& s) {')
    assert 'TRAIN_LAUNCH_CAP * train_slot_bytes(B)' in _function(train, '\nint stage_inputs(Step& s) {')
    assert 'rec_abort[TRAIN_LAUNCH_CAP]' in csrc['train_state.h'] and train.count('getenv("CASV_') == 2 == _function(train, 'static TrainSwitches read_train_switches(').count('getenv("CASV_')
    for n, code in csrc.items():
        if n != 'train_plan.h':
            assert not re.search(r'TRAIN_LAUNCH_CAP\s*=|TRAIN_MIN_CUS\s*=|ATTN_DEFER_MAX_T\s*=|_counter_bytes\(int B\)', code), n


_LAUNCH_SITE = r'layers_forward\(m, f, \d|launch_train_attention_cell\(|launch_train_attention_cell_bwd\(|layers_backward\(m, \w+, \d'


def _step_functions(train):
    """{name: body} of train.hip's functions that take the step's view."""
    return {name: _function(train, head) for head, name in re.findall(r'^((?:static )?\w+ (\w+)\(Step&? s[,)])', train, re.M)}


def _launch_sites(fns, name):
    """The launch sites of a function of the step in the order of its text, those of the step's functions it calls in their place."""
    out = []
    body = fns[name][fns[name].index('{'):]
    for hit in re.finditer(r'%s|\b(%s)\(s[,)]' % (_LAUNCH_SITE, '|'.join(fns)), body):
        out += _launch_sites(fns, hit.group(1)) if hit.group(1) else [hit.group(0)]
    return out


def test_restated_order_of_launches_is_train_hip():
    train = _src('train.hip')
    fns = _step_functions(train)
    attempt = fns['train_attempt']
    phases = re.findall(r'if \(int rc = (\w+)\(s[,)]', attempt)
    assert phases == ['plan_buffers', 'stage_inputs', 'forward_layers', 'forward_cell', 'loss_head', 'backward_cell', 'backward_layers',
                      'update']
    assert set(phases) < set(fns) and not re.search(_LAUNCH_SITE, attempt)
    step = _function(train, 'extern "C" int casv_train_step(')
    assert step.count('train_attempt(s, ') == 1 and 'casv_train_step(m' not in step.split('{', 1)[1] and not re.search(_LAUNCH_SITE, step)
    order = _launch_sites(fns, 'train_attempt')
    assert order == ['layers_forward(m, f, 2',                                      # encoder layer 1, both directions
                     'layers_forward(m, f, 2', 'layers_forward(m, f, 1',            # deep: layer n's directions, then decoder layer n - 1 alone
                     'layers_forward(m, f, 2',                                      # else: encoder layer n beside decoder layer n - 1
                     'launch_train_attention_cell(', 'launch_train_attention_cell_bwd(',
                     'layers_backward(m, one, 1', 'layers_backward(m, pair, 2',     # deep: decoder layer n alone, then layer n + 1's directions
                     'layers_backward(m, pair, 2',                                  # else: decoder layer n beside encoder layer n + 1
                     'layers_backward(m, pair, 2']                                  # encoder layer 1
    assert len(re.findall(_LAUNCH_SITE, train)) == len(order)       # (no launch site outside the attempt's phases)
    assert _launch_sites(fns, 'forward_layers') == order[:4] and _launch_sites(fns, 'forward_cell') == order[4:5]
    assert _launch_sites(fns, 'backward_cell') == order[5:6] and _launch_sites(fns, 'backward_layers') == order[6:]
    fwd, bwd = fns['forward_layers'], fns['backward_layers']
    assert 'for (int n = 2; n <= D && deep; ++n)' in fwd and 'for (int n = 2; n <= D && !deep; ++n)' in fwd
    assert fwd.index('for (int n = 2; n <= D && deep; ++n)') < fwd.index('for (int n = 2; n <= D && !deep; ++n)')
    assert 'for (int n = D - 1; n >= 1 && deep; --n)' in bwd and 'for (int n = D - 1; n >= 1 && !deep; --n)' in bwd
    assert bwd.index('for (int n = D - 1; n >= 1 && deep; --n)') < bwd.index('for (int n = D - 1; n >= 1 && !deep; --n)')
    from oracle import ModelConfig
    plain = tf.sites(ModelConfig(depth=3, width=128, voc_size=40), 5, 7)
    assert [(k, l) for k, l, _ in plain] == [('rec', ('enc1_fw', 'enc1_bw')), ('rec', ('enc2', 'dec1')), ('rec', ('enc3', 'dec2')),
                                             ('cell', ('dec3',)), ('cell_bwd', ('dec3',)), ('rec_bwd', ('dec2', 'enc3')),
                                             ('rec_bwd', ('dec1', 'enc2')), ('rec_bwd', ('enc1_fw', 'enc1_bw'))]
    assert [n for _, _, n in plain] == [(5, 5), (5, 7), (5, 7), (7,), (7,), (7, 5), (7, 5), (5, 5)]


def test_the_statistics_are_documented():
    with open(os.path.join(ROOT, 'include', 'cor_asv_ann_hip.h')) as f:
        text = f.read()
    stat = text[text.index('Statistics of the last call'):text.index('int casv_get_stat')]
    assert '"train_persistent_launches"' in stat and '"train_give_ups"' in stat
    assert 'strcmp(key, "train_persistent_launches")' in _src('engine.hip') and 'strcmp(key, "train_give_ups")' in _src('engine.hip')


# ------------------------------------------------------------------------------------------------------------------ 3. the bounds can fail
@pytest.mark.parametrize('name', tf.MUTATED)
def test_mutations_exceed_the_noise_bound(name):
    fc = tf.BY_NAME[name]
    cfg, w, inputs, _, o64, o32 = tf.oracles(fc)
    frozen = fc[0][10]
    muts = dict(gn.mutations(cfg, w, inputs, frozen))
    muts.update(tf.form_mutations(cfg, w, inputs, frozen))
    assert set(muts) >= {'target_weight_zeroed', 'last_step_removed', 'row_clamp_leaks', 'shorter_job_cut'}
    assert ('cell_mask_flipped' in muts) == fc[0][7]
    for mut, got in muts.items():
        excess = gn.excess(gn.ratios(got, o32, o64))
        assert excess >= 10, (mut, excess)


# ------------------------------------------------------------------------------------------------------------------ 4. the units
@pytest.mark.parametrize('fc', tf.ALL, ids=tf.IDS)
def test_noise_units_are_not_degenerate(fc):
    """The fp32 oracle measured in its own units is at 1 (below 1 where a unit is floored): the bounds leave the device C_RMS and
    C_MAX of those.  Apart from att_bv's, at most a quarter of a case's units may sit on the floor (train_form_cases.floored_units)."""
    cfg, w, inputs, _, o64, o32 = tf.oracles(fc)
    r = gn.ratios(o32, o32, o64)
    assert all(a <= 1 + 1e-12 and b <= 1 + 1e-12 for a, b in r.values())
    on, n = tf.floored_units(o32, o64)
    assert all(abs(r[k][1] - 1) < 1e-12 for k in r if k not in on)
    on = [k for k in on if k not in gn.ZERO_GRADIENTS]
    assert len(on) <= n / 4, on
    assert np.isfinite(o64[0]) and o64[1] > 0
