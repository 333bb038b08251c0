"""The GEMM launch decision as a pure function (csrc/gemm_plan.h), pinned on the CPU.

A stand-alone driver (tests/gemm_plan_driver.cpp: only gemm_plan.h and the standard library, built with the host compiler) plans
every case of tests/gemm_plan_cases.py; every record it prints -- forms, grids, LDS sizes, cut rows, moved pointers, clears -- must
equal the table, which was recorded from the launchers before the planner existed.  Source checks hold the structure: the planner
knows nothing of the device or the environment, and the five GEMM files only run plans."""
import collections
import os
import re
import shutil
import subprocess

import pytest

from tests import gemm_plan_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'cor_asv_ann_amd', 'csrc')
GEMM_FILES = ('gemm.hip', 'gemm_split.hip', 'gemm_skinny.hip', 'gemm_tn.hip', 'gemm_tn_split.hip')
FORMS = {'g128', 'g128x2', 's128', 'k32', 'k64', 's256'}
TN_KERNELS = {'tn', 'tns', 'tn_part', 'tns_part'}


@pytest.fixture(scope='module')
def planned(tmp_path_factory):
    """{case name: the records the planner gives}"""
    cxx = os.environ.get('CXX') or next((c for c in ('c++', 'g++', 'clang++') if shutil.which(c)), None)
    if not cxx or not shutil.which(cxx):
        pytest.skip('no host compiler')
    exe = str(tmp_path_factory.mktemp('gemm_plan') / 'driver')
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', os.path.join(ROOT, 'tests', 'gemm_plan_driver.cpp'), '-o', exe], check=True)
    text = ''.join(line + '\n' for _, line in gc.CASES)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    got, name = {}, None
    for line in out.splitlines():
        if line.startswith('case '):
            name = line[5:]
            assert name not in got, name
            got[name] = []
        else:
            got[name].append(line)
    return got


def test_every_case_plans_as_the_launchers_did(planned):
    assert list(planned) == [name for name, _ in gc.CASES]
    wrong = [(name, gc.EXPECTED[name], planned[name]) for name, _ in gc.CASES if planned[name] != gc.EXPECTED[name]]
    assert not wrong, 'first of %d: %r' % (len(wrong), wrong[0])


def _launches(name):
    """[(form, [rows of each job])] of a forward case"""
    return [(rec.split()[1], [int(m) for m in re.findall(r'\| M=(\d+)', rec)]) for rec in gc.EXPECTED[name] if rec.startswith('L ')]


def test_the_table_covers_every_form_and_both_outcomes_of_both_cuts():
    names = [name for name, _ in gc.CASES]
    assert len(names) == len(set(names)) >= 240 and set(names) == set(gc.EXPECTED)
    assert all(gc.EXPECTED[name] for name in names)
    forms = collections.Counter(rec.split()[1] for recs in gc.EXPECTED.values() for rec in recs if rec[0] in 'LT')
    assert set(forms) == FORMS | TN_KERNELS, forms
    assert min(forms.values()) >= 5, forms
    # the cut of a partial round of 128x128 tiles: taken, switched off, and left alone for a last round that is three quarters full
    assert _launches('train_round_cut') == [('g128', [49152]), ('k32', [2560])]
    assert _launches('train_round_cut_64_rows') == [('g128', [49152]), ('k64', [3072])]
    assert _launches('train_round_cut_off') == [('g128', [51712])]
    assert _launches('train_round_three_quarters_full') == [('g128', [61952])]
    # the cut of a 256x256 grid: a partial round, a tail that goes as 256x256 again, a ragged block, no cut
    assert _launches('split2_10240') == [('s256', [8192]), ('s128', [2048])]
    assert _launches('split2_12288') == [('s256', [8192]), ('s256', [4096])]
    assert _launches('split2_10300') == [('s256', [8192]), ('s128', [2108])]
    assert _launches('split2_tail_cut_off') == [('s256', [10240])]
    assert _launches('split2_nact_group_does_not_divide') == [('s256', [10240])]
    assert _launches('split2_four_jobs_all_cut') == [('s256', [8192] * 4), ('s128', [2048] * 4)]
    assert any(rec.startswith('C ') for recs in gc.EXPECTED.values() for rec in recs if recs[-1].startswith('L '))
    assert any(rec.startswith('C ') for recs in gc.EXPECTED.values() for rec in recs if recs[-1].startswith('=>'))
    # a device with other CUs decides otherwise -- except the ordered weight gradient, whose bits must follow from the shape alone
    assert gc.EXPECTED['split2_12288_ncu304'] != gc.EXPECTED['split2_12288'] != gc.EXPECTED['split2_12288_ncu64']
    assert gc.EXPECTED['tn_split_form_ncu64'] != gc.EXPECTED['tn_split_form_arith2']
    for shape in gc.TN_SHAPES:
        assert gc.EXPECTED['tn_%s_ncu64_ordered' % shape] == gc.EXPECTED['tn_%s_arith2_ordered' % shape] == gc.EXPECTED['tn_%s_ncu304_ordered' % shape]


# ---- the structure ----
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _code(text):
    """the text without its comments"""
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', text, flags=re.S))


def _definitions(text):
    """[(name, body)] of the top-level definitions: from a line at column 0 that is no comment, directive or closing brace to the
    next closing brace at column 0; name = the identifier in front of the first parenthesis of the signature (None: there is none),
    body = the lines behind the signature."""
    out, lines = [], None
    for line in text.split('\n'):
        if lines is None and line and not line[0].isspace() and not line.startswith(('//', '#', '}')):
            lines = []
        if lines is not None:
            lines.append(line)
            if line.startswith('}') or (len(lines) == 1 and line.rstrip().endswith((';', '}'))):
                sig = 1 if lines[0].startswith('template') and len(lines) > 1 else 0
                m = re.match(r'[^(]*?(\w+)\(', lines[sig])
                out.append((m.group(1) if m else None, '\n'.join(lines[sig + 1:])))
                lines = None
    return out


def test_the_planner_knows_neither_the_device_nor_the_environment():
    for name in ('gemm_plan.h', 'gemm_args.h'):
        code = _code(_src(name))
        assert not re.search(r'\bhip', code, re.I) and 'getenv' not in code and '#include "common.h"' not in code, name
    assert re.findall(r'#include [<"]([^>"]+)[>"]', _src('gemm_plan.h')) == ['gemm_args.h', 'algorithm']
    assert '#include "gemm_args.h"' in _src('common.h') and 'struct GemmArgs' not in _src('common.h')


def test_the_gemm_files_only_run_plans():
    holders = []
    for name in GEMM_FILES:
        code = _code(_src(name))
        assert 'thread_local' not in code and 'hipGetDeviceProperties' not in code, name
        holders += [(name, fn) for fn, body in _definitions(code) if 'getenv' in body]
    assert holders == [('gemm.hip', 'gemm_switches_from_env')]
    # no launch path comes back to the launcher or to itself: the plan is a flat list
    for name in GEMM_FILES + ('gemm_plan.h',):
        code = _code(_src(name))
        for fn, body in _definitions(code):
            assert fn is None or not re.search(r'\b%s\(' % fn, body), (name, fn)
        assert len(re.findall(r'\blaunch_gemm_batch\(', code)) == (2 if name == 'gemm.hip' else 0), name      # its definition, and launch_gemm
    everything = ''.join(_code(_src(name)) for name in GEMM_FILES + ('gemm_plan.h',))
    assert len([line for line in everything.split('\n') if 'xr <= 8' in line]) == 1                 # the XCD tile-order search
    assert len([line for line in everything.split('\n') if 'ktiles / 64' in line]) == 1             # the K-share rule of the weight gradients
    assert len(re.findall(r'hipFuncSetAttribute', everything)) == 0 and _src('common.h').count('hipFuncSetAttribute(') == 1
    assert len(re.findall(r'hipMemset', everything)) == 0


def test_the_thread_locals_are_gone():
    common = _src('common.h')
    for name in ('gemm_split_enter', 'gemm_split_bf16', 'gemm_ordered_enter', 'gemm_ordered'):
        assert not re.search(r'\b%s\b' % name, common), name
    assert 'GemmContext gemm' in _src('engine.h')
    assert 'std::to_string(m->gemm.arithmetic)' in _src('decode.hip')        # the step graph's key
