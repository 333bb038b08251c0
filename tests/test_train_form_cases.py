"""Without a GPU: the case table of tests/train_form_cases.py reaches every instantiation the train step's dispatchers name, its
restated form decision (train_form) uses the constants and conditions the .hip sources hold, the noise bounds would see a
persistent kernel that gets a row-block edge or a job's last step wrong, and no case measures against a degenerate noise unit."""
import os
import re

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
def test_restated_constants_and_conditions_are_the_sources():
    rec, bwd, top, topb, train = (_src(n) for n in ('train_persist.hip', 'train_persist_bwd.hip', 'train_persist_top.hip',
                                                     'train_persist_topb.hip', 'train.hip'))
    # row blocks
    for text, name in ((rec, 'RBM'), (bwd, 'QBM'), (top, 'TBM'), (topb, 'VBM')):
        assert int(re.search(r'constexpr int %s = (\d+)' % name, text).group(1)) == tf.ROW_BLOCK
    # workgroups of a launch and the workgroups per CU the residency query is capped at
    grids = {'rec': (rec, 'rec_grid', 'RBM', 'ra.njobs * '), 'rec_bwd': (bwd, 'recb_grid', 'QBM', 'ra.njobs * '),
             'cell': (top, 'top_grid', 'TBM', ''), 'cell_bwd': (topb, 'topb_grid', 'VBM', '')}
    for kind, (text, fn, bm, jobs) in grids.items():
        body = _function(text, 'template <int NT> static int %s(' % fn)
        assert 'const int grid = %s((ra.B + %s - 1) / %s) * NT;' % (jobs, bm, bm) in body, kind
        m = re.search(r'return grid <= persist_blocks_per_cu\((\w+)<NT>, 0, (\d+)\) \* ncu \? grid : 0;', body)
        assert m and m.group(1) == tf.KERNEL[kind] and int(m.group(2)) == tf.BLOCKS_PER_CU[kind], kind
    # the conditions and the switch labels of the four dispatchers (and of the launchers: the same labels)
    labels = lambda body: tuple(int(x) for x in re.findall(r'case (\d+):', body))
    body = _function(rec, 'int train_recurrence_grid(')
    assert 'if (ra.W % 32 || ra.njobs < 1 || ra.njobs > 2 || ra.B < 1) return 0;' in body and 'switch (ra.W / 32)' in body
    widths = re.search(r'#define CASV_REC_WIDTHS\(X\)((?: X\(\d+\))+)', rec).group(1)
    assert tuple(int(x) for x in re.findall(r'X\((\d+)\)', widths)) == tf.NT['rec']
    assert 'CASV_REC_WIDTHS(CASV_REC_CASE)' in body and 'CASV_REC_WIDTHS(CASV_REC_CASE)' in _function(rec, 'void launch_train_recurrence(')
    assert len(re.findall(r'train_recurrence_kernel<', rec)) == 2        # (the grid and the launcher: no instantiation beside the list)
    body = _function(bwd, 'int train_recurrence_bwd_grid(')
    assert 'if (ra.W % 128 || ra.njobs < 1 || ra.njobs > 2 || ra.B < 1) return 0;' in body and 'switch (ra.W / 32)' in body
    assert labels(body) == labels(_function(bwd, 'void launch_train_recurrence_bwd(')) == tf.NT['rec_bwd']
    body = _function(top, 'int train_attention_cell_grid(')
    assert 'if (ra.W != ra.C || ra.B < 1 || ra.U < 1) return 0;' in body and 'switch (ra.W / 32 * (ra.W % 32 == 0))' in body
    assert labels(body) == labels(_function(top, 'void launch_train_attention_cell(')) == tf.NT['cell']
    body = _function(topb, 'int train_attention_cell_bwd_grid(')
    assert 'if (ra.W != ra.C || ra.W % 128 || ra.B < 1 || ra.U < 1 || ra.ab.C > 1024) return 0;' in body
    assert labels(body) == labels(_function(topb, 'void launch_train_attention_cell_bwd(')) == tf.NT['cell_bwd']
    assert labels(_function(topb, 'bool train_attention_cell_bwd_rows_fit(')) == tf.NT['cell_bwd']
    assert labels(_function(topb, 'void launch_train_attention_cell_bwd_rows(')) == tf.NT['cell_bwd']
    assert tf.SPLIT_KERNEL + '<' in topb
    # every instantiation of the five kernels goes through those switches
    for text, kernel in ((bwd, tf.KERNEL['rec_bwd']), (top, tf.KERNEL['cell']), (topb, tf.KERNEL['cell_bwd']), (topb, tf.SPLIT_KERNEL)):
        assert set(int(x) for x in re.findall(r'%s<(\d+)>' % kernel, text)) <= set(tf.NT['rec']), kernel
    # train.hip: ONE place that decides (persist_slot) and ONE that counts (persist_launched), called from the four sites; the cap as
    # one named constant; the cell's and the backward's own conditions
    cap = 'REC_LAUNCH_CAP'
    assert len(re.findall(r'constexpr int %s = (\d+);' % cap, train)) == 1
    assert int(re.search(r'constexpr int %s = (\d+);' % cap, train).group(1)) == tf.CAP
    cond = 'if (m->persist_mode != 0 && !m->deterministic && ts->rec_skip == 0 && ts->rec_launches < %s && m->ncu >= %d) {' % (cap, tf.MIN_CUS)
    assert train.count(cond) == 1 and cond in _function(train, 'static unsigned* persist_slot(casv_model* m, TrainState* ts) {')
    assert re.findall(r'rec_launches < \w+', train) == ['rec_launches < ' + cap] and train.count('persist_mode != 0') == 1
    assert 'const unsigned* rec_abort[%s]' % cap in train and len(re.findall(r'rec_launches\+\+', train)) == 1
    assert 'rec_launches++' in _function(train, 'static void persist_launched(TrainState* ts, unsigned* slot, size_t counter_bytes) {')
    sites = {'layers_backward': 'static int layers_backward(', 'layers_forward': 'static int layers_forward(',
             'forward_cell': 'static int forward_cell(', 'cell_backward_persistent': 'static int cell_backward_persistent('}
    for name, head in sites.items():
        body = _function(train, head)
        assert len(re.findall(r'unsigned\* slot = persist_slot\(m, ts\)', body)) == 1 and body.count('ra.counters = slot;') == 1, name
        assert len(re.findall(r'persist_launched\(ts, slot, %s\(B\)\);' % tf.COUNTER_BYTES[name], body)) == 1, name
    assert len(re.findall(r'persist_slot\(m, ts\)', train)) == 4 and len(re.findall(r'persist_launched\(ts, slot, ', train)) == 4
    # one slot size: the largest of the four kinds' counters, for the addresses, the allocation and the clear
    body = _function(train, 'static size_t persist_slot_bytes(int B) {')
    assert all(body.count(fn + '(B)') == 1 for fn in tf.COUNTER_BYTES.values()) and body.count('std::max(') == 3
    assert 'persist_slot_bytes(ts->B) * ts->rec_launches' in _function(train, 'static unsigned* persist_slot(')
    assert 'ENS(ts->rec_cnt, %s * persist_slot_bytes(B))' % cap in _function(train, 'static int plan_buffers(Step& s) {')
    assert 'hipMemsetAsync(ts->rec_cnt.p, 0, %s * persist_slot_bytes(B), st)' % cap in _function(train, 'static int stage_inputs(Step& s) {')
    assert train.count('persist_slot_bytes(') == 4
    assert 'const int grid = top.hs_ld == W ? train_attention_cell_grid(ra, m->ncu) : 0' in _function(train, sites['forward_cell'])
    body = _function(train, sites['layers_backward'])
    assert 'plain = plain && l.kr == W;' in body and 'const int grid = plain ? train_recurrence_bwd_grid(ra, m->ncu) : 0;' in body
    assert ('ra.split_a = split_opt && !ts->split_off && train_attention_cell_bwd_rows_fit(ra) ? 1 : 0;'
            in _function(train, sites['cell_backward_persistent']))


_LAUNCH_SITE = r'layers_forward\(m, f, \d|launch_train_attention_cell\(|launch_train_attention_cell_bwd\(|layers_backward\(m, \w+, \d'


def _step_functions(train):
    """{name: body} of train.hip's functions that take the step's view."""
    return {name: _function(train, head) for head, name in re.findall(r'^(static \w+ (\w+)\(Step&? s[,)])', train, re.M)}


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
