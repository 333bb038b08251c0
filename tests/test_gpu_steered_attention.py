"""The rejection rule of the beam search, the attention at window widths 1 to 4 and saturated attention energies on a real MI355X,
on models whose attention rows are steered by hand (tests/steer_models.py; tests/test_steer_models.py shows on the CPU that the
table's results are decided by the rule and not by rounding, and that each flipped rule changes a named output).

- Preconditions, one casv_decoder_step per case: the alignment rows are fl32(1/k) on the allowed positions of the window and exact
  zeros elsewhere, bit for bit the fp32 oracle's; the distribution is the tie model's (the context does not reach it).
- casv_decode_beam against tie_models.search for every line and result, by tests/test_gpu_beam_ties.py's rules, the dense alignments
  exact; each line alone, the batch and the batch reversed bit for bit; arithmetic 0 and 2.
- casv_decode_greedy on the same tracks, modes 0 and 1, persistent and per step: rows and window stores exact, the forms bit-equal.
- casv_score_targets at window widths 1 to 5 (random weights: the real encoder cannot feed a steered att_U; the smallest model case
  and the block case, whose fused form runs the persistent top cell), attention rows against
  the stepped float64 restatement, the window form equal to the dense rows.
- Widths 1 to 4 under the unchanged noise bounds of tests/decode_noise_cases.py and tests/grad_noise_cases.py.
- Saturated energies: every energy of the window underflowing, one or two overflowing, and -- the declared deviation -- an overflow
  outside the window."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

os.environ.setdefault('CASV_POISON', '1')      # read once by the library, at its first allocation

from oracle import ModelConfig
from oracle.decode import OracleModel
from tests import decode_noise_cases as dn
from tests import grad_noise_cases as gn
from tests import score_cases as sc
from tests.steer_models import CASES, BY_NAME, GATE_OFF, run_search, steered_weights
from tests import tie_models
from tests.tie_models import against_the_oracle as _against_the_oracle, bits as _bits, same_bits as _same_bits, uniform_weights

_oracle = {}


def _expected(case):
    if case.name not in _oracle:
        m = case.model()
        enc_in, idx, src_rej = case.inputs(m)
        want = [(res, stats, [list(r[4]) for r in res], trace) for res, stats, trace in run_search(case)]
        _oracle[case.name] = dict(m=m, enc=case.encoder_outputs(m), src_rej=src_rej, want=want)
    return _oracle[case.name]


def _engine(case, arithmetic, lm=False):
    from cor_asv_ann_amd.engine import HipEngine
    eng = HipEngine(case.cfg.depth, case.cfg.width, case.V, window_width=case.window)
    eng.set_weights(case.weights())
    eng.set_option('arithmetic', arithmetic)
    eng.set_option('lm_predict', int(lm))
    return eng


def _install(eng, e, rows):
    enc = e['enc']
    eng.set_encoder_outputs(enc[0][rows], [x[rows] for x in enc[1:-1]], a0=enc[-1][rows], src_rej=e['src_rej'][rows])


def _same_or_nan(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(_bits(a)[~np.isnan(a)], _bits(b)[~np.isnan(b)])


# ------------------------------------------------------------------------------------------------------------------ preconditions
@pytest.mark.parametrize('name', [c.name for c in CASES])
def test_a_steered_step_gives_the_exact_rows(name):
    case = BY_NAME[name]
    e = _expected(case)
    m, enc = e['m'], e['enc']
    B, T, V = len(case.lines), case.T, case.V
    every = list(range(B))
    eng = _engine(case, 0)
    try:
        _install(eng, e, every)
        _, states = eng.encoder_outputs()
        line = np.arange(B, dtype=np.int32)
        p1, st1 = eng.decoder_step(line, np.zeros((B, V), np.float32), states, enc[-1])
        p2, st2 = eng.decoder_step(line, p1, st1[:-1], st1[-1])
    finally:
        eng.close()
    q1, ost1 = m.step(np.zeros((B, V), np.float32), enc[0], enc[1:])
    q2, ost2 = m.step(q1, enc[0], ost1)
    for j in range(B):
        tp = np.float32(1.0 if case.a0[j] is None else case.a0[j] + 1.0)
        assert np.array_equal(_bits(st1[-1][j]), _bits(case.expected_row(j, tp))), (name, j)
    assert np.array_equal(_bits(st1[-1]), _bits(ost1[-1])) and np.array_equal(_bits(st2[-1]), _bits(ost2[-1]))
    for a in (st1[-1], st2[-1]):            # identical rows give identical bits: one value per row beside the zeros
        assert all(len(np.unique(_bits(r[r != 0]))) == 1 for r in a)
    if case.family == 'uniform':
        assert np.array_equal(_bits(p1), _bits(np.full((B, V), np.float32(1) / np.float32(V), np.float32)))
    else:
        tie = OracleModel(case.cfg, {k: v.astype(np.float32) for k, v in tie_models.Case.weights(case).items()})
        t1, _ = tie.step(np.zeros((B, V), np.float32), enc[0], enc[1:])
        assert np.array_equal(_bits(q1), _bits(t1))                        # (the oracle's: the context does not reach the distribution)
        assert np.allclose(p1, t1, rtol=2e-4, atol=0) and len(np.unique(p1[0])) > 1
    assert np.array_equal(_bits(p2), _bits(p1))                             # another alignment, another context: the same distribution


# ------------------------------------------------------------------------------------------------------------------ the search
def _decode(eng, case, e, rows):
    """-> per line a list of results, each a dict of arrays cut to the result's length (tests/test_gpu_beam_ties.py, _decode)."""
    B, MR = len(rows), case.max_results
    _install(eng, e, rows)
    res = eng.decode_beam(want_align=True, **case.decoder_kwargs())
    S = res['idx'].shape[1]
    lo, w = eng.alignments_sparse(B * MR, S)
    out = []
    for j in range(B):
        found = []
        for k in range(min(int(res['n_found'][j]), MR, 64)):
            r = j * MR + k
            n = int(res['len'][r])
            found.append(dict(idx=res['idx'][r, :n].copy(), prob=res['prob'][r, :n].copy(), rej=res['rej'][r, :n].copy(),
                              score=res['score'][r].copy(), align=res['align'][r, :n].copy(), lo=lo[r, :n].copy(), w=w[r, :n].copy()))
        out.append(dict(n_found=int(res['n_found'][j]), n_steps=int(res['n_steps'][j]), results=found,
                        empty=res['len'][j * MR + len(found):(j + 1) * MR].copy()))
    return out


@pytest.mark.parametrize('name,arithmetic', [(c.name, a) for c in CASES for a in (0, 2)])
def test_the_search_on_a_steered_model_equals_the_oracle(name, arithmetic):
    case = BY_NAME[name]
    e = _expected(case)
    B = len(case.lines)
    eng = _engine(case, arithmetic, case.lm)
    try:
        batch = _decode(eng, case, e, list(range(B)))
        alone = [_decode(eng, case, e, [j])[0] for j in range(B)]
        backwards = _decode(eng, case, e, list(range(B))[::-1])[::-1]
    finally:
        eng.close()
    _against_the_oracle(case, batch, e['want'], e['m'].mapping[0])
    for dev, (res, _, _, _) in zip(batch, e['want']):
        for d, r in zip(dev['results'], res):
            a = np.asarray(r[3], np.float32).reshape(len(r[0]), case.T)
            assert np.array_equal(_bits(d['align']), _bits(a)), (name, r[0])         # the dense alignments: exact
    _same_bits(batch, alone, 'each line alone')
    _same_bits(batch, backwards, 'lines reversed')


# ------------------------------------------------------------------------------------------------------------------ greedy
def _greedy_walk(m, enc, S):
    """The alignment rows of decode_batch_greedy's S steps (the full distribution fed back) -> (B, S, T)."""
    p, states, rows = np.zeros((enc[0].shape[0], m.voc_size), np.float32), list(enc[1:]), []
    for _ in range(S):
        p, states = m.step(p, enc[0], states)
        rows.append(states[-1])
    return np.stack(rows, axis=1)


def _greedy(eng, e, rows, mode, S, T):
    import cor_asv_ann_amd._native as nv
    _install(eng, e, rows)
    B = len(rows)
    out = dict(idx=np.full((B, S), -7, np.int32), prob=np.full((B, S), -7, np.float32), len=np.full(B, -7, np.int32),
               align=np.full((B, S, T), -7, np.float32))
    rc = eng.lib.casv_decode_greedy(eng.handle, mode, S, nv.ptr(out['idx']), nv.ptr(out['prob']), nv.ptr(out['len']), nv.ptr(out['align']))
    assert rc in (0, nv.CASV_ERR_NAN), eng.lib.casv_last_error()
    out['lo'], out['w'] = eng.alignments_sparse(B, S)
    return out


def _greedy_rows_equal(got, want, T, where):
    """The dense rows against the oracle's, exact, NaN where it has NaN; the window form against the dense rows."""
    for j, n in enumerate(got['len']):
        n = int(n)
        a = got['align'][j, :n]
        assert _same_or_nan(a, want[j, :n]), (where, j)
        for s in range(n):
            lo = int(got['lo'][j, s])
            if np.isnan(a[s]).all():
                assert lo == -1, (where, j, s, lo)            # -1: the row is NaN at all T positions
                continue
            k = min(got['w'].shape[2], T - lo)
            window = np.zeros(T, np.float32)
            window[lo:lo + k] = got['w'][j, s, :k]
            assert lo >= 0 and _same_or_nan(window, a[s]) and not got['w'][j, s, k:].any(), (where, j, s)


@pytest.mark.parametrize('name', [c.name for c in CASES])
def test_greedy_on_the_same_tracks_is_exact_in_every_form(name):
    case = BY_NAME[name]
    e = _expected(case)
    B, T = len(case.lines), case.T
    S = 2 * T
    want = _greedy_walk(e['m'], e['enc'], S)
    eng = _engine(case, 0)
    got = {}
    try:
        for persistent in (1, 0):
            eng.set_option('persistent', persistent)
            for mode in (0, 1):
                got[persistent, mode] = _greedy(eng, e, list(range(B)), mode, S, T)
    finally:
        eng.close()
    for (persistent, mode), g in got.items():
        assert mode == 1 or (g['len'] == S).all()
        _greedy_rows_equal(g, want, T, (name, persistent, mode))
    for mode in (0, 1):
        a, b = got[1, mode], got[0, mode]
        assert np.array_equal(a['len'], b['len'])
        for j, n in enumerate(a['len']):
            assert np.array_equal(a['idx'][j, :n], b['idx'][j, :n]) and np.array_equal(a['lo'][j, :n], b['lo'][j, :n])
            for key in ('prob', 'align', 'w'):
                assert _same_or_nan(a[key][j, :n], b[key][j, :n]), (name, mode, j, key)


# ------------------------------------------------------------------------------------------------------------------ scoring forward
# the smallest model case, and the one whose top cell has a persistent form (train_attention_cell_kernel takes widths 128, 256 and
# 512 only: at any other width the "fused" form steps the top cell kernel by kernel, like "stepwise")
SCORE_CASES = {'smallest': sc.MODEL_CASES[0], 'block': sc.BLOCK_CASE}
SCORE_FORMS = {'fused': (('persistent', -1),), 'stepwise': (('persistent', 0),), 'deterministic': (('deterministic', 1),)}


def _score_setup(which, window, bv=None):
    from cor_asv_ann_amd.engine import HipEngine
    c = SCORE_CASES[which]
    mc = sc.model_case(c)
    cfg = ModelConfig(depth=c[0], width=c[1], voc_size=c[2], window=window)
    w = dict(mc['w'])
    if bv is not None:
        w['att_bv'] = np.full_like(w['att_bv'], bv)
    return mc, cfg, w, lambda: HipEngine(c[0], c[1], c[2], window_width=window)


def _score(make, w, form, mc, which):
    """casv_score_targets with the dense rows -> (logp, rows, lo, window weights); the fused form of the block case ran its top
    cell as a persistent launch."""
    import cor_asv_ann_amd._native as nv
    eng = make()
    try:
        eng.set_weights(w)
        for k, v in SCORE_FORMS[form]:
            eng.set_option(k, v)
        logp, _, _, _, _, align = eng.score_targets(mc['enc_idx'], mc['enc_val'], mc['din'], mc['dout'], want_align=True)
        if which == 'block' and form == 'fused':
            assert eng.stat('train_persistent_launches') >= 1
        if form == 'stepwise':
            assert eng.stat('train_persistent_launches') == 0
        K = 2 * eng.window_width + 1
        lo, ww = np.empty(align.shape[:2], np.int32), np.empty(align.shape[:2] + (K,), np.float32)
        nv.check(eng.lib.casv_score_get_alignments_sparse(eng.handle, K, nv.ptr(lo), nv.ptr(ww)))
    finally:
        eng.close()
    return logp, align, lo, ww


def _window_form_equals(align, lo, w, where):
    B, U, T = align.shape
    K = w.shape[2]
    for b in range(B):
        for u in range(U):
            if lo[b, u] < 0:
                assert np.isnan(align[b, u]).all() and np.isnan(w[b, u]).all(), (where, b, u)
                continue
            n = min(K, T - lo[b, u])
            dense = np.zeros(T, np.float32)
            dense[lo[b, u]:lo[b, u] + n] = w[b, u, :n]
            assert _same_or_nan(dense, align[b, u]) and not w[b, u, n:].any(), (where, b, u)         # the SAME call: bit for bit


@pytest.mark.parametrize('form', list(SCORE_FORMS))
@pytest.mark.parametrize('window', [1, 2, 3, 4, 5])
@pytest.mark.parametrize('which', list(SCORE_CASES))
def test_the_scoring_forward_at_every_window_width(which, window, form):
    mc, cfg, w, make = _score_setup(which, window)
    rows64 = sc.stepped(cfg, {k: v.astype(np.float64) for k, v in w.items()}, mc['enc_in'], mc['dec_in'], np.float32)[1]
    _, align, lo, ww = _score(make, w, form, mc, which)
    assert np.allclose(align, rows64, rtol=2e-4, atol=2e-6), np.abs(align - rows64).max()
    assert ((align != 0).sum(axis=2) <= 2 * window + 1).all() and (lo >= 0).all()
    _window_form_equals(align, lo, ww, (which, window, form))


# ------------------------------------------------------------------------------------------------------------------ noise bounds
WIDTH_STEP_CASES = [(dn.STEP_CASES[0], 2), (dn.STEP_CASES[0], 4), (dn.STEP_CASES[1], 2), (dn.STEP_CASES[1], 4)]
WIDTH_GRAD_CASES = [(c, win) for c in gn.CASES if c[0] in ('d2_w32_b4_m', 'd3_w128_b37_m') for win in (1, 3)]


def test_the_width_cases_are_the_ones_named():
    assert [c[0][0] for c in WIDTH_STEP_CASES] == ['r37_d2_w256_v40'] * 2 + ['r1000_d1_w512_v256'] * 2
    assert sorted({c[0][0] for c in WIDTH_GRAD_CASES}) == ['d2_w32_b4_m', 'd3_w128_b37_m'] and len(WIDTH_GRAD_CASES) == 4


@pytest.mark.parametrize('case,window', WIDTH_STEP_CASES, ids=['%s_win%d' % (c[0], win) for c, win in WIDTH_STEP_CASES])
def test_decoder_steps_at_widths_2_and_4_within_the_noise_bounds(case, window):
    cfg, w, (line, enc, states, a, p_in) = dn.build_step(case, window=window)
    assert cfg.window == window
    engs = {ar: dn.step_engine(cfg, w, enc, ar) for ar in (0, 2)}
    try:
        for s in range(case[7]):
            o32 = dn.oracle_step(cfg, w, line, enc, states, a, p_in, np.float32)
            o64 = dn.oracle_step(cfg, w, line, enc, states, a, p_in, np.float64)
            assert (np.nan_to_num(o32['a']) != 0).sum(axis=1).max() <= 2 * window + 1
            for ar, eng in engs.items():
                got = dn.device_step(eng, line, states, a, p_in)
                assert not dn.nan_mismatch(got, o32), (s, ar, dn.nan_mismatch(got, o32))
                r = dn.ratios(got, o32, o64)
                print('window_width_noise step %s window %d step %d arithmetic %d: %s' % (
                    case[0], window, s, ar, ' '.join('%s %.3f/%.3f' % (k, v[0], v[1]) for k, v in sorted(r.items()))))
                bad = {k: v for k, v in r.items() if v[0] > dn.C_RMS or v[1] > dn.C_MAX}
                assert not bad, (s, ar, bad)
            states, a, p_in = dn.next_inputs(cfg, o32)
    finally:
        for eng in engs.values():
            eng.close()


@pytest.mark.parametrize('case,window', WIDTH_GRAD_CASES, ids=['%s_win%d' % (c[0], win) for c, win in WIDTH_GRAD_CASES])
def test_the_train_step_at_widths_1_and_3_within_the_noise_bounds(case, window):
    cfg, w, inputs, batch = gn.build(case, window=window)
    assert cfg.window == window
    o64, o32 = gn.oracle(cfg, w, inputs, np.float64), gn.oracle(cfg, w, inputs, np.float32)
    for path in ('fused', 'stepwise'):
        for det in (0, 1):
            got = gn.device(case, w, batch, path, det, window=window)
            r = gn.ratios(got, o32, o64)
            worst = max(((k, v) for k, v in r.items() if k not in gn.ZERO_GRADIENTS), key=lambda kv: max(kv[1][0] / gn.C_RMS, kv[1][1] / gn.C_MAX))
            print('window_width_noise train %s window %d %s deterministic %d: worst %s %.3f/%.3f, largest rms %.3f, largest max %.3f' % (
                case[0], window, path, det, worst[0], worst[1][0], worst[1][1],
                max(v[0] for k, v in r.items() if k not in gn.ZERO_GRADIENTS), max(v[1] for k, v in r.items() if k not in gn.ZERO_GRADIENTS)))
            bad = {k: v for k, v in r.items() if k not in gn.ZERO_GRADIENTS and (v[0] > gn.C_RMS or v[1] > gn.C_MAX)}
            assert not bad, (path, det, bad)
            for k in gn.ZERO_GRADIENTS:
                assert gn.within_old_bound(got[2][k], o64[2][k], o64[1]), (path, det, k)


# ------------------------------------------------------------------------------------------------------------------ saturated energies
SAT_T, SAT_V, SAT_P = 24, 16, 10         # a0 one-hot at 10: t' = 11, the window 6..16
GATE_OVER = 20.0                         # energy +750: exp overflows to inf
# line -> {position: gate}; every other position is GATE_OFF
SAT_TRACKS = {
    'plain': {8: 0.0, 11: 0.0, 12: 0.0, 20: 0.0},
    'a_all_underflow': {2: 0.0, 20: 0.0},                           # allowed positions outside the window only
    'b_one_overflow': {8: 0.0, 11: GATE_OVER, 12: 0.0},
    'c_two_overflows': {6: GATE_OVER, 9: 0.0, 16: GATE_OVER},
    'd_overflow_outside': {8: 0.0, 11: 0.0, 12: 0.0, 3: GATE_OVER, 20: GATE_OVER},
}
SAT_LINES = list(SAT_TRACKS)


def _saturated(masked=False):
    """cfg, weights, encoder outputs (lines, T, C), a0 rows.  masked: the overflow outside the window gated off."""
    cfg = ModelConfig(depth=2, width=32, voc_size=SAT_V)
    w = steered_weights(cfg, uniform_weights(cfg))
    enc = np.zeros((len(SAT_LINES), SAT_T, cfg.ctx_width), np.float32)
    enc[:, :, 0] = GATE_OFF
    for j, name in enumerate(SAT_LINES):
        for s, g in SAT_TRACKS[name].items():
            if not (masked and g == GATE_OVER and abs(SAT_P + 1 - s) > cfg.window):
                enc[j, s, 0] = g
    a0 = np.zeros((len(SAT_LINES), SAT_T), np.float32)
    a0[:, SAT_P] = 1.0
    return cfg, w, enc, a0


def _sat_engine(cfg, w, enc, a0, rows):
    from cor_asv_ann_amd.engine import HipEngine
    eng = HipEngine(cfg.depth, cfg.width, cfg.voc_size)
    eng.set_weights(w)
    eng.set_option('arithmetic', 0)
    eng.set_encoder_outputs(enc[rows], [np.zeros((len(rows), cfg.width), np.float32)] * (2 * cfg.depth), a0=a0[rows])
    return eng


def _sat_step(masked):
    cfg, w, enc, a0 = _saturated(masked)
    B = len(SAT_LINES)
    line = np.arange(B, dtype=np.int32)
    states = [np.zeros((B, cfg.width), np.float32)] * (2 * cfg.depth)
    p_in = np.zeros((B, SAT_V), np.float32)
    return cfg, w, enc, a0, line, states, p_in, dn.oracle_step(cfg, w, line, enc, states, a0, p_in, np.float32)


def test_saturated_energies_inside_the_window_give_the_oracles_rows():
    """(a) every energy of the window at -750: 0/0, the whole row NaN and the context with it; (b), (c) one or two at +750: inf/inf
    there, 0 at the others."""
    cfg, w, enc, a0, line, states, p_in, o32 = _sat_step(False)
    eng = _sat_engine(cfg, w, enc, a0, list(range(len(SAT_LINES))))
    try:
        got = dn.device_step(eng, line, states, a0, p_in)
    finally:
        eng.close()
    j = {name: k for k, name in enumerate(SAT_LINES)}
    abc = [j['plain'], j['a_all_underflow'], j['b_one_overflow'], j['c_two_overflows']]
    assert np.isnan(o32['a'][j['a_all_underflow']]).all()
    assert list(np.flatnonzero(np.isnan(o32['a'][j['b_one_overflow']]))) == [11] and not np.nan_to_num(o32['a'][j['b_one_overflow']]).any()
    assert list(np.flatnonzero(np.isnan(o32['a'][j['c_two_overflows']]))) == [6, 16]
    assert np.isnan(o32['a'][j['d_overflow_outside']]).all()                  # the reference: inf * 0 poisons the row
    for k in o32:
        assert np.array_equal(np.isnan(got[k][abc]), np.isnan(o32[k][abc])), k
    assert _same_or_nan(got['a'][abc], o32['a'][abc])
    for name in ('a_all_underflow', 'b_one_overflow', 'c_two_overflows'):       # the context is NaN: it reaches every output
        assert all(np.isnan(got[k][j[name]]).all() for k in ('probs', 'h2', 'c2')), name
    assert np.array_equal(_bits(got['probs'][j['plain']]), _bits(np.full(SAT_V, np.float32(1) / np.float32(SAT_V), np.float32)))


def test_deviation_an_overflow_outside_the_window_is_not_looked_at():
    """(d), the declared deviation: exp(+750) = inf at a position OUTSIDE the window makes the reference's
    row NaN through inf * 0; the device evaluates the window only.  Its row is the oracle's with that position masked before the exp."""
    cfg, w, enc, a0, line, states, p_in, masked = _sat_step(True)
    eng = _sat_engine(cfg, w, enc, a0, list(range(len(SAT_LINES))))
    try:
        got = dn.device_step(eng, line, states, a0, p_in)
    finally:
        eng.close()
    d = SAT_LINES.index('d_overflow_outside')
    assert not np.isnan(masked['a'][d]).any() and list(np.flatnonzero(masked['a'][d])) == [8, 11, 12]
    for k in masked:
        assert _same_or_nan(got[k][d], masked[k][d]) if k == 'a' else np.array_equal(np.isnan(got[k][d]), np.isnan(masked[k][d])), k


@pytest.mark.parametrize('name', ['a_all_underflow', 'b_one_overflow', 'c_two_overflows'])
def test_saturated_energies_through_the_greedy_decoder(name):
    """One line through the persistent decoder and the per-step kernels: the rows the oracle's, NaN where it has NaN; a row that is
    all NaN has lo = -1 in the window form; the two forms bit-equal (att_window_next carries the NaNs in registers)."""
    cfg, w, enc, a0 = _saturated()
    r = [SAT_LINES.index(name)]
    m = OracleModel(cfg, w)
    S = 6
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        want = _greedy_walk(m, [enc[r]] + [np.zeros((1, cfg.width), np.float32)] * (2 * cfg.depth) + [a0[r]], S)
    assert np.isnan(want[0, 1:]).all()                                          # behind a NaN t' every window is empty
    e = dict(enc=[enc] + [np.zeros((len(SAT_LINES), cfg.width), np.float32)] * (2 * cfg.depth) + [a0],
             src_rej=np.full((len(SAT_LINES), SAT_T), -1, np.int32))
    got = {}
    eng = _sat_engine(cfg, w, enc, a0, r)
    try:
        for persistent in (1, 0):
            eng.set_option('persistent', persistent)
            got[persistent] = _greedy(eng, e, r, 0, S, SAT_T)
    finally:
        eng.close()
    for persistent, g in got.items():
        assert g['len'][0] == S
        _greedy_rows_equal(g, want, SAT_T, (name, persistent))
        assert (g['lo'][0, 1:] == -1).all() and (g['lo'][0, 0] == -1) == (name == 'a_all_underflow')
    for key in ('align', 'w', 'prob'):
        assert _same_or_nan(got[1][key], got[0][key]), key
    assert np.array_equal(got[1]['lo'], got[0]['lo'])


@pytest.mark.parametrize('which', list(SCORE_CASES))
def test_saturated_energies_through_the_scoring_forward(which):
    """The real encoder cannot feed a gate track, so the bias saturates every energy at once: att_bv = -750 is (a) at every step --
    all-NaN rows, lo = -1, NaN log-probabilities -- in the three forms, the fused one (on the block case train_attention_cell_kernel:
    the row written by one of a row's two waves, the next window carried in registers) bit for bit the stepwise one.
    (att_bv = +750 would put inf at the positions outside the window too: the declared deviation, not (b) or (c).)"""
    mc, cfg, w, make = _score_setup(which, 5, -750.0)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        rows32 = sc.stepped(cfg, w, mc['enc_in'], mc['dec_in'])[1]
    assert np.isnan(rows32).all()
    got = {form: _score(make, w, form, mc, which) for form in SCORE_FORMS}
    for form, (logp, align, lo, ww) in got.items():
        assert np.isnan(align).all() and (lo == -1).all() and np.isnan(ww).all(), form
        assert np.isnan(logp).all(), form         # (the head's rule: a row with a NaN logit scores NaN, tests/score_cases.py _head)
    for form in ('stepwise', 'deterministic'):
        for x, y in zip(got['fused'], got[form]):
            assert np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(x[~np.isnan(x)], y[~np.isnan(y)]), form


OVER_SCALE, OVER_BV = 2050.0, 455.0


@pytest.mark.parametrize('form', list(SCORE_FORMS))
def test_overflows_through_the_scoring_forward(form):
    """(b) and (c) through the real encoder: no gate track can be fed, but att_va scaled by 2050 with att_bv = 455 spreads the first
    step's energies of the block case so far that of its 37 lines some have one position of the window above exp's overflow (88.7),
    some two and some none -- every energy at least 2 away from the overflow and the underflow threshold, none overflowing outside
    the window (asserted on the float64 energies).  On the lines with an overflow the rows are exact: NaN there, 0 elsewhere, and NaN
    at every later step.  The other lines' rows are finite at the first step; their values carry the scaled energies' rounding and
    are not compared."""
    from oracle.model import encode
    mc, cfg, w, make = _score_setup('block', 5)
    w['att_va'] = (w['att_va'] * np.float32(OVER_SCALE)).astype(np.float32)
    w['att_bv'] = np.full_like(w['att_bv'], OVER_BV)
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    outs = encode(cfg, w64, mc['enc_in'].astype(np.float64))
    T = outs[0].shape[1]
    energy = np.tanh((outs[2 * cfg.depth - 1] @ w64['att_Wa'] + w64['att_bUW'])[:, None, :] + outs[0] @ w64['att_U']) @ w64['att_va'] + OVER_BV
    inside = np.abs(1.0 - np.arange(T)) <= cfg.window
    assert (np.abs(energy - 88.72) >= 2).all() and (np.abs(energy + 103.97) >= 2).all() and not (energy[:, ~inside] > 88.72).any()
    overflows = (energy[:, inside] > 88.72).sum(axis=1)
    assert {0, 1, 2} <= set(overflows.tolist())
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        rows32 = sc.stepped(cfg, w, mc['enc_in'], mc['dec_in'])[1]
    assert np.array_equal(np.isnan(rows32[:, 0]).sum(axis=1), overflows)
    sat = overflows > 0
    logp, align, lo, ww = _score(make, w, form, mc, 'block')
    assert _same_or_nan(align[sat], rows32[sat])
    assert np.isnan(align[sat][:, 1:]).all() and (lo[sat][:, 1:] == -1).all() and (lo[sat][:, 0] == 0).all()
    assert not np.isnan(align[~sat][:, 0]).any() and not align[~sat][:, 0, ~inside].any()
    assert np.isnan(logp[sat][mc['dout'][sat] >= 0]).all()
    _window_form_equals(align, lo, ww, form)
