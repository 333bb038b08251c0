"""The plans of the decode path's persistent launches (csrc/persist_plan.h) pinned without a device.

A stand-alone driver (tests/persist_plan_driver.cpp: only persist_plan.h and the standard library, built with the host compiler,
-Wall -Werror, and once more under the address and undefined-behaviour sanitizers) plans every case of tests/persist_form_cases.py
on 256 CUs and on four other CU counts, under every value of the option "persistent"; every record must equal the Python
restatement.  At 256 CUs with the workgroups per CU recorded from an MI355X the table must reach every form the kernels have, and
every case must be persistent exactly under the option values it is marked for.  Source checks tie the header's constants to the
kernels' and keep the arithmetic out of the hosts."""
import os
import re
import shutil
import subprocess

import pytest

from tests import persist_form_cases as pf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'cor_asv_ann_amd', 'csrc')
DRIVER = os.path.join(ROOT, 'tests', 'persist_plan_driver.cpp')
CUS = (256, 304, 128, 64, 48)                # the MI355X, a larger part, smaller ones, one below PERSIST_MIN_CUS
OPTIONS = (-1, 0, 1)
RESIDENCIES = (None, (1, 1), (2, 2))         # the recorded figures, and either figure for every kernel


def _cxx():
    cxx = os.environ.get('CXX') or next((c for c in ('c++', 'g++', 'clang++') if shutil.which(c)), None)
    if not cxx or not shutil.which(cxx):
        pytest.skip('no host compiler')
    return cxx


def _extra():
    """Lines beside the table: (key, driver line, record the restatement gives)."""
    out = []
    d9 = pf.DEPTH_9
    for p in (-1, 1):
        out.append(('depth9_enc|%d' % p, 'E x %d %d 0 0 %d 256 2 %d 0' % (d9['d'], d9['W'], d9['B'], p),
                    pf.encoder_record(pf.encoder_form(d9['d'], d9['W'], d9['B'], per_cu=2, persistent=p))))
        out.append(('depth9_split|%d' % p, 'E x %d %d 0 0 %d 256 2 %d 1' % (d9['d'], d9['W'], d9['B'], p),
                    pf.encoder_record(pf.encoder_form(d9['d'], d9['W'], d9['B'], per_cu=2, persistent=p, split=True))))
        out.append(('depth9_dec|%d' % p, 'D x %d %d %d %d %d 256 2 %d 0' % (d9['d'], d9['W'], pf.padded_voc(d9['V']), d9['W'], d9['B'], p),
                    pf.decoder_record(pf.decoder_form(d9['d'], d9['W'], d9['V'], d9['B'], per_cu=2, persistent=p))))
        out.append(('split_arith_dec|%d' % p, 'D x 2 64 64 64 20 256 2 %d 2' % p,
                    pf.decoder_record(pf.decoder_form(2, 64, 50, 20, per_cu=2, persistent=p, arithmetic=2))))
        out.append(('residual_d3|%d' % p, 'E x 3 64 1 0 20 256 2 %d 0' % p,
                    pf.encoder_record(pf.encoder_form(3, 64, 20, per_cu=2, persistent=p, residual=True))))
        out.append(('residual_d2|%d' % p, 'E x 2 64 1 0 20 256 2 %d 0' % p,
                    pf.encoder_record(pf.encoder_form(2, 64, 20, per_cu=2, persistent=p, residual=True))))
        out.append(('deep_d2|%d' % p, 'E x 2 64 0 1 20 256 2 %d 1' % p,
                    pf.encoder_record(pf.encoder_form(2, 64, 20, per_cu=2, persistent=p, split=True, deep=True))))
        out.append(('deep_d2_dec|%d' % p, 'D x 2 64 64 128 20 256 2 %d 0' % p,
                    pf.decoder_record(pf.decoder_form(2, 64, 50, 20, per_cu=2, persistent=p, deep=True))))
        for B in (4096, 4097):
            out.append(('b%d_enc|%d' % (B, p), 'E x 2 32 0 0 %d 256 2 %d 0' % (B, p),
                        pf.encoder_record(pf.encoder_form(2, 32, B, per_cu=2, persistent=p))))
            out.append(('b%d_dec|%d' % (B, p), 'D x 2 32 64 32 %d 256 2 %d 0' % (B, p),
                        pf.decoder_record(pf.decoder_form(2, 32, 50, B, per_cu=2, persistent=p))))
        for B in (256, 257):
            out.append(('split_b%d|%d' % (B, p), 'E x 2 64 0 0 %d 256 2 %d 1' % (B, p),
                        pf.encoder_record(pf.encoder_form(2, 64, B, per_cu=2, persistent=p, split=True))))
    out.append(('failed_query_dec', 'D x 2 64 64 64 20 256 0 -1 0', pf.decoder_record(pf.decoder_form(2, 64, 50, 20, per_cu=0))))
    out.append(('failed_query_enc', 'E x 2 64 0 0 20 256 0 -1 0', pf.encoder_record(pf.encoder_form(2, 64, 20, per_cu=0))))
    return out


def _table():
    """[(key, driver line, record the restatement gives)] of every case on every CU count, option value and residency."""
    rows = []
    for case in pf.CASES:
        for cus in CUS:
            for p in OPTIONS:
                for res in RESIDENCIES:
                    enc, dec = pf.forms(case, cus=cus, persistent=p, per_cu=res)
                    lines = pf.driver_lines(case, cus, p, per_cu=res)
                    key = '%s|%d|%d|%s' % (case.name, cus, p, res)
                    rows.append((key + '|E', lines[0], pf.encoder_record(enc)))
                    if dec is not None:
                        rows.append((key + '|D', lines[1], pf.decoder_record(dec)))
    return rows + _extra()


def _run(exe, rows):
    text = ''.join(line + '\n' for _, line, _ in rows)
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return [line for line in out.stdout.splitlines() if not line.startswith('case ')]


@pytest.fixture(scope='module')
def rows():
    return _table()


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('persist_plan') / 'driver')
    subprocess.run([_cxx(), '-std=c++17', '-O1', '-Wall', '-Werror', DRIVER, '-o', exe], check=True)
    return exe


def test_the_plans_equal_the_restatement_on_every_case_and_cu_count(driver, rows):
    got = _run(driver, rows)
    assert len(got) == len(rows) and len(set(k for k, _, _ in rows)) == len(rows)
    wrong = [(k, line, want, g) for (k, line, want), g in zip(rows, got) if g != want]
    assert not wrong, 'first of %d: %r' % (len(wrong), wrong[0])
    # the CU counts decide otherwise, and below 64 CUs nothing is persistent
    by_key = {k: g for (k, _, _), g in zip(rows, got)}
    assert by_key['d2_w256_v256_b272|256|-1|None|D'] != by_key['d2_w256_v256_b272|304|-1|None|D'] != by_key['d2_w256_v256_b272|128|-1|None|D']
    assert all('reason=cus' in g for (k, _, _), g in zip(rows, got) if '|48|' in k and '|0|' not in k)
    assert all('reason=off' in g for (k, _, _), g in zip(rows, got) if '|0|' in k)


def test_the_driver_is_clean_under_the_host_sanitizers(tmp_path, driver, rows):
    cxx = _cxx()
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    flags = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer']
    if subprocess.run([cxx] + flags + [str(probe), '-o', str(tmp_path / 'probe')], capture_output=True).returncode != 0:
        pytest.skip('the host compiler has no sanitizer runtime')
    exe = str(tmp_path / 'driver_san')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Werror'] + flags + [DRIVER, '-o', exe], check=True)
    assert _run(exe, rows) == _run(driver, rows)


def _at_256():
    return {c.name: pf.forms(c, persistent=1) for c in pf.CASES}


def test_every_case_has_its_residency_on_record():
    for c in pf.CASES:
        if c.arith == 0:
            lds = pf.enc_lds(c.d, c.W)[1]
            assert lds > pf.LDS_LIMIT or lds in pf.RESIDENCY['encode'], c.name
            if c.dec is not None:
                lds = pf.dec_lds(c.d, c.W, c.V)[2]
                assert lds > pf.LDS_LIMIT or lds in pf.RESIDENCY['decode'], c.name
    assert pf.RESIDENCY['split'] == {pf.SPLIT_LDS: 2}
    for kernel in ('decode', 'encode'):           # two workgroups per CU up to about 75 KB of staged rows, one above
        table = pf.RESIDENCY[kernel]
        assert all(table[lds] == (2 if lds <= 73984 else 1) for lds in table) and min(table.values()) == 1, kernel


def test_the_table_reaches_every_form_on_256_cus():
    f = _at_256()
    dec = {n: d for n, (_, d) in f.items() if d is not None and d['applies']}
    enc = {n: e for n, (e, _) in f.items() if e['form'] != 'none'}
    D = lambda n: dec[n]
    E = lambda n: enc[n]
    # ---- decoder: tiles per workgroup
    assert (D('d2_w256_v256_b256')['lstm_own'], D('d2_w256_v256_b256')['g_lstm'], D('d2_w256_v256_b256')['per_cu']) == (1, 256, 2)
    assert (D('d2_w256_v256_b272')['lstm_own'], D('d2_w256_v256_b272')['lstm_round']) == (2, 'partial')
    assert (D('d2_w256_v256_b512')['lstm_own'], D('d2_w256_v256_b512')['lstm_round']) == (2, 'full')
    assert D('d2_w256_v40_b528')['lstm_own'] == 3
    for n in ('d2_w512_v256_b80', 'd2_w512_v256_b128'):
        assert (D(n)['lstm_own'], D(n)['per_cu'], D(n)['g_lstm']) == (2, 1, 128), n
    assert (D('d2_w512_v256_b80')['lstm_round'], D('d2_w512_v256_b128')['lstm_round']) == ('partial', 'full')
    # ---- plain tasks per workgroup, idle waves
    assert D('d2_w256_v256_b256')['plain_own'] == 1 and D('d2_w256_v256_b256')['g_plain'] == 128
    for n in ('d2_w256_v256_b272', 'd2_w256_v256_b512', 'd2_w512_v256_b128'):
        assert D(n)['plain_own'] >= 2, n
    assert D('d2_w96_v257_b17')['query_idle'] and D('d2_w96_v257_b17')['logits_idle']
    assert not D('d2_w256_v256_b256')['query_idle'] and not D('d2_w256_v256_b256')['logits_idle']
    # ---- attention
    assert D('d2_w256_v256_b512')['attention'] == 'rows' and D('d2_w256_v256_b512')['att_own'] == 1
    assert D('d2_w512_v256_b128')['attention_why'] == ('width', 'ctx')          # (C >= W: a wide model is past both limits)
    assert D('d1_w256_v40_b40')['attention_why'] == ('ctx',)
    assert D('d2_w256_v40_b528')['attention_why'] == ('rows',) and D('d2_w256_v40_b528')['att_own'] == 2
    for n in ('d2_w512_v256_b80', 'd2_w512_v256_b128', 'd1_w256_v40_b40', 'd2_w256_v40_b528'):
        assert pf.BY_NAME[n].modes == (0, 1), n
    # ---- softmax statistics, depths, rows
    assert {d['stats'] for d in dec.values()} == {'quarter_full', 'quarter', 'wave'}
    assert {pf.BY_NAME[n].d for n in dec} >= {1, 2, 8}
    assert {pf.BY_NAME[n].B for n in dec} >= {1, 15, 16, 17}
    # ---- the LDS edge
    assert D('d2_w768_v40_b16')['lds'] == 147712 and E('d2_w768_v40_b16')['per_cu'] == 1 and pf.enc_lds(2, 768)[1] == 147712
    e800, d800 = f['d2_w800_v40_b16']
    assert (e800['reason'], d800['reason'], d800['lds']) == ('lds', 'lds', 153856) and pf.enc_lds(2, 800)[1] == 153856
    # ---- chain encoder
    assert (E('d2_w256_v256_b256')['own1'], E('d2_w256_v256_b256')['ownn']) == (1, 1)
    assert (E('d2_w256_v256_b272')['own1'], E('d2_w256_v256_b272')['round1']) == (2, 'partial')
    assert (E('d2_w256_v256_b512')['own1'], E('d2_w256_v256_b512')['round1']) == (2, 'full')
    assert E('d4_w256_v40_b512')['ownn'] == 3
    assert (E('d8_w128_v40_b1168')['own1'], E('d8_w128_v40_b1168')['ownn']) == (3, pf.ENC_MAX_TILES)
    e = f['d8_w128_v40_b1184'][0]
    assert (e['form'], e['reason'], e['ownn']) == ('none', 'own', pf.ENC_MAX_TILES + 1)
    assert E('d1_w256_v40_b40')['roundn'] == '-'
    assert pf.BY_NAME['d2_w64_v50_b20_t1'].L == 0 and pf.BY_NAME['d3_w64_v50_b20_t2'].L == 1
    assert (E('d2_w512_v256_b128')['per_cu'], E('d2_w512_v256_b128')['grid'], E('d2_w512_v256_b128')['own1']) == (1, 256, 2)
    # ---- split encoder
    assert (E('split_d2_w128_v64_b40')['own1'], E('split_d2_w128_v64_b40')['ownn']) == (1, 1)
    assert (E('split_d8_w512_v40_b160')['ownn'], E('split_d8_w512_v40_b160')['grid']) == (2, 512)
    assert E('split_d8_w128_v40_b2336')['ownn'] == pf.SPLIT_MAX_TILES
    e = f['split_d8_w128_v40_b2368'][0]
    assert (e['form'], e['reason'], e['ownn']) == ('none', 'own', pf.SPLIT_MAX_TILES + 1)
    assert E('split_d1_w128_v64_b33')['roundn'] == '-' and pf.BY_NAME['split_d2_w64_v50_b20_t1'].L == 0
    # every case that is not about the length has 6 to 10 source positions
    assert all(6 <= c.L + 1 <= 10 for c in pf.CASES if not c.name.endswith(('_t1', '_t2')))


def test_every_case_is_persistent_under_the_option_values_it_is_marked_for():
    for c in pf.CASES:
        for p in OPTIONS:
            enc, dec = pf.forms(c, persistent=p)
            assert (enc['form'] != 'none') == pf.expected(c.enc, p), (c.name, p, enc)
            if dec is not None:
                assert dec['applies'] == pf.expected(c.dec, p), (c.name, p, dec)
    assert {c.enc for c in pf.CASES} == {'default', 'forced', 'none'} and {c.dec for c in pf.CASES} == {'default', 'forced', 'none', None}
    d9 = pf.DEPTH_9
    assert pf.encoder_form(d9['d'], d9['W'], d9['B'], persistent=1, per_cu=2)['reason'] == 'depth'
    assert pf.decoder_form(d9['d'], d9['W'], d9['V'], d9['B'], persistent=1, per_cu=2)['reason'] == 'depth'


# ---- the structure ----
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _code(text):
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', text, flags=re.S))


def _constant(text, name):
    m = re.search(r'constexpr \w+ %s = ([^;]+);' % name, text)
    assert m, name
    return eval(m.group(1), {'__builtins__': {}}, {'PS_BUF_BYTES': 8 * 3 * 32 * 32})


def test_the_header_is_pure_and_its_constants_are_the_kernels_and_the_tables():
    plan = _src('persist_plan.h')
    code = _code(plan)
    assert not re.search(r'\bhip', code, re.I) and 'getenv' not in code
    assert re.findall(r'#include [<"]([^>"]+)[>"]', plan) == ['algorithm', 'cstddef']
    assert re.findall(r'#include [<"]([^>"]+)[>"]', open(DRIVER).read())[0] == '../cor_asv_ann_amd/csrc/persist_plan.h'
    assert _constant(plan, 'PERSIST_ENC_MAX_TILES') == _constant(_src('persist.hip'), 'PENC_MAXT') == pf.ENC_MAX_TILES
    assert _constant(plan, 'PERSIST_SPLIT_MAX_TILES') == _constant(_src('persist_split.hip'), 'PS_MAXT') == pf.SPLIT_MAX_TILES
    assert _constant(_src('persist_split.hip'), 'PS_LDS_BYTES') == pf.SPLIT_LDS
    assert _constant(plan, 'PERSIST_LDS_LIMIT') == pf.LDS_LIMIT and _code(_src('persist.hip')).count('lds > 150 * 1024') == 4
    assert (_constant(plan, 'PERSIST_MIN_CUS'), _constant(plan, 'PERSIST_MAX_DEPTH')) == (pf.MIN_CUS, pf.MAX_DEPTH)
    assert (_constant(plan, 'PERSIST_MAX_ROWS_FORCED'), _constant(plan, 'PERSIST_MAX_ROWS_DEFAULT'), _constant(plan, 'PERSIST_MAX_OWN_DEFAULT'),
            _constant(plan, 'PERSIST_SPLIT_DEFAULT_ROWS')) == (pf.ROWS_FORCED, pf.ROWS_DEFAULT, pf.OWN_DEFAULT, pf.SPLIT_DEFAULT_ROWS)
    # the counters' layout is persist_host.h's; the kernels index the same counters per row block
    assert '(n * 32 + 32) * sizeof(unsigned)' in _src('persist_host.h') and '(counters * 32 + 32) * sizeof(unsigned)' in plan
    assert 'const int NCNT = D + 3;' in _src('persist.hip') and _src('persist.hip').count('const int NCNT = D + 1;') == 1
    assert 'const int NCNT = D + 1;' in _src('persist_split.hip')
    reasons = [[r.strip().lower() for r in body.split(',')] for body in re.findall(r'enum Reason \{([^}]+)\}', plan)]
    assert reasons == [list(pf.DEC_REASONS), list(pf.ENC_REASONS)]


def test_the_hosts_only_ask_for_the_residency_and_run_the_plan():
    dec, enc = _code(_src('decode.hip')), _code(_src('encoder.hip'))
    assert 'plan_persist_decode(' in dec and 'plan_persist_encode(' in enc
    assert dec.count('persist_decode_blocks_per_cu(') == 1 and enc.count('persist_encode_blocks_per_cu(') == 1 == enc.count('persist_split_encode_blocks_per_cu(')
    for word in ('wgslots', 'nq4', 'ntile', 'own1', 'ownn', '4096', '<= 512', '150 * 1024'):
        assert word not in dec and word not in enc, word
    assert 'ncu < 64' not in dec and 'ncu < 64' not in enc


def test_the_statistics_are_documented():
    keys = ('decoder_persistent', 'decode_give_ups', 'decoder_persist_per_cu', 'decoder_persist_g_lstm', 'decoder_persist_g_att',
            'decoder_persist_g_plain', 'encoder_persist_per_cu', 'encoder_persist_grid')
    with open(os.path.join(ROOT, 'include', 'cor_asv_ann_hip.h')) as f:
        text = ' '.join(f.read().replace(' * ', ' ').split())
    stat = text[text.index('Statistics of the last call'):text.index('int casv_get_stat')]
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as f:
        integration = f.read()
    for key in keys:
        assert 'strcmp(key, "%s")' % key in _src('engine.hip'), key
        assert key in integration, key
    for key in ('"decoder_persistent"', '"decode_give_ups"', '"decoder_persist_per_cu"', '"decoder_persist_g_lstm"', '"encoder_persist_per_cu"',
                '"encoder_persist_grid"'):
        assert key in stat, key
