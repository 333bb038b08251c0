"""The greedy decode's pick rules on a real MI355X, on models with exact ties, saturated rows and NaN rows
(tests/greedy_tie_cases.py): casv_decode_greedy against the fp32 oracle for EVERY line of every case, in both modes -- on these
models the pick is decided by the bookkeeping and not by rounding (tests/test_greedy_tie_cases.py shows that on the CPU, and that
each flipped rule changes an expected output).  The call goes through the binding with the test's own arrays, so that indices,
probabilities and lengths survive a CASV_ERR_NAN return.

Exact: the return code, out_len, every reported index (mode 0: all S steps of every row; mode 1: each line's reported part),
probabilities that are fl32(1/V), 1.0 or 0.0, and where NaNs fall.  Other probabilities and the alignments (dense, and the window
form equal to the dense rows bit for bit): rtol 2e-4 + atol 2e-6, the suite's tolerance (test_gpu_parity.py).
Forms: `persistent` 0 (softmax_kernel) and 1 (row_stats_quarter<true>, <false>, row_stats by V) under arithmetic 0, bit for bit
with each other; `persistent` 0 under arithmetic 2; each line alone, the batch and the batch reversed, bit for bit.

Preconditions come first, so that a failure points at the pick and not at the model: one casv_decoder_step gives bitwise-equal
probabilities at the tied indices, exactly fl32(1/V) on the uniform family, and the same bits at step 2 as at step 1."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

os.environ.setdefault('CASV_POISON', '1')      # read once by the library, at its first allocation

from tests.greedy_tie_cases import CASES, BY_NAME, MODES, NEGATIVE_ROWS, greedy_form, run

RT, AT = 2e-4, 2e-6
_oracle = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _expected(case):
    """-> dict: the fp32 model, the input indices, what the decode starts from, per mode the restated decode (the oracle's: the
    CPU test), and for a NaN case the same with that row finite."""
    if case.name not in _oracle:
        m = case.model()
        _oracle[case.name] = dict(m=m, idx=case.inputs(m)[1], enc=case.encoder_outputs(m), want={mode: run(case, mode) for mode in MODES})
    return _oracle[case.name]


def _engine(case, arithmetic):
    from cor_asv_ann_amd.engine import HipEngine
    eng = HipEngine(case.cfg.depth, case.cfg.width, case.V)
    eng.set_weights(case.weights())
    eng.set_option('arithmetic', arithmetic)
    return eng


def _install(eng, case, idx, enc, rows):
    if case.explicit:
        eng.set_encoder_outputs(enc[0][rows], [e[rows] for e in enc[1:-1]])
    else:
        eng.encode(idx[rows])


def _decode(eng, case, mode):
    """casv_decode_greedy on what is installed -> dict(rc, idx, prob, len, align, lo, w)."""
    import cor_asv_ann_amd._native as nv
    B, S, T = eng.B, case.S, case.T
    out = dict(idx=np.full((B, S), -7, np.int32), prob=np.full((B, S), -7, np.float32), len=np.full(B, -7, np.int32),
               align=np.full((B, S, T), -7, np.float32))
    out['rc'] = eng.lib.casv_decode_greedy(eng.handle, mode, S, nv.ptr(out['idx']), nv.ptr(out['prob']), nv.ptr(out['len']),
                                           nv.ptr(out['align']))
    assert out['rc'] in (0, nv.CASV_ERR_NAN), eng.lib.casv_last_error()
    out['lo'], out['w'] = eng.alignments_sparse(B, S)
    return out


def _rows_of(parts):
    """Decodes of single lines -> one dict as of the batch (rc: the worst)."""
    out = {k: np.concatenate([p[k] for p in parts]) for k in ('idx', 'prob', 'len', 'align', 'lo', 'w')}
    out['rc'] = min(p['rc'] for p in parts)
    return out


def _reordered(d, order):
    return dict({k: d[k][order] for k in ('idx', 'prob', 'len', 'align', 'lo', 'w')}, rc=d['rc'])


def _same_bits(a, b, mode, what):
    assert a['rc'] == b['rc'] and np.array_equal(a['len'], b['len']), what
    for j, n in enumerate(a['len']):
        n = int(n)            # (mode 1: rows keep stepping after their line has ended; only the reported part counts)
        assert np.array_equal(a['idx'][j, :n], b['idx'][j, :n]) and np.array_equal(a['lo'][j, :n], b['lo'][j, :n]), (what, mode, j)
        for key in ('prob', 'align', 'w'):
            assert np.array_equal(_bits(a[key][j, :n]), _bits(b[key][j, :n])), (what, mode, j, key)


def _against_the_oracle(case, dev, want, mode, rows, what):
    import cor_asv_ann_amd._native as nv
    T, V = case.T, case.V
    pinned = _bits(np.array([np.float32(1) / np.float32(V), 1.0, 0.0], np.float32))
    raised = bool(want['raised'][rows].any())
    assert dev['rc'] == (nv.CASV_ERR_NAN if raised else 0), (what, mode, dev['rc'])
    assert np.array_equal(dev['len'], want['length'][rows]), (what, mode, dev['len'], want['length'][rows])
    for j, r in enumerate(rows):
        where = (what, case.name, mode, r)
        n = int(want['length'][r])
        assert n == case.S or mode == 1
        assert np.array_equal(dev['idx'][j, :n], want['idx'][r, :n]), (where, dev['idx'][j, :n], want['idx'][r, :n])
        p, q = dev['prob'][j, :n], want['prob'][r, :n].astype(np.float32)
        assert np.array_equal(np.isnan(p), np.isnan(q)), (where, p, q)
        exact = np.isin(_bits(q), pinned)
        assert np.array_equal(_bits(p)[exact], _bits(q)[exact]), (where, p, q)
        assert np.allclose(p, q, rtol=RT, atol=AT, equal_nan=True), (where, p, q)
        a, b = dev['align'][j, :n], want['align'][r, :n].astype(np.float32)
        assert np.array_equal(np.isnan(a), np.isnan(b)), where
        assert np.allclose(a, b, rtol=RT, atol=AT, equal_nan=True), where
        window = np.zeros_like(a)
        for s in range(n):
            lo = int(dev['lo'][j, s])
            if lo < 0:
                assert np.isnan(a[s]).all(), where          # -1: the row is all NaN
                window[s] = np.nan
                continue
            k = min(dev['w'].shape[2], T - lo)
            window[s, lo:lo + k] = dev['w'][j, s, :k]
            assert not dev['w'][j, s, k:].any(), where
        assert np.array_equal(_bits(window)[~np.isnan(a)], _bits(a)[~np.isnan(a)]) and np.array_equal(np.isnan(window), np.isnan(a)), where


def _preconditions(eng, case, idx, enc):
    B, T, V = case.B, case.T, case.V
    _install(eng, case, idx, enc, list(range(B)))
    _, states = eng.encoder_outputs()
    line = np.arange(B, dtype=np.int32)
    p1, st1 = eng.decoder_step(line, np.zeros((B, V), np.float32), states, np.zeros((B, T), np.float32))
    neg = [r for r in NEGATIVE_ROWS if r < B] if case.explicit else []
    pos = [r for r in range(B) if r not in neg and r != case.nan_row]
    if case.family == 'uniform':
        assert np.array_equal(_bits(p1), _bits(np.full((B, V), np.float32(1) / np.float32(V), np.float32)))
    for rows, key in ((pos, 'tie'), (neg, 'neg')):
        tie = list(case.promises.get(key, ()))
        if len(tie) > 1 and rows:
            assert (_bits(p1[rows][:, tie]) == _bits(p1[rows][:, tie[:1]])).all(), key       # identical E rows: identical probabilities
            others = [v for v in range(V) if v not in tie]
            assert not others or (p1[rows][:, tie[0]] > p1[rows][:, others].max(axis=1)).all(), key
    if case.nan_row is not None:
        assert np.isnan(p1[case.nan_row]).all()
    assert np.isfinite(p1[pos + neg]).all()
    p2, st2 = eng.decoder_step(line, p1, st1[:-1], st1[-1])
    ok = pos + neg
    assert np.array_equal(_bits(p2[ok]), _bits(p1[ok]))                 # the state is held: fast_sigmoid(30) == 1, fast_tanh(0) == 0
    for a, b in zip(st1[1:-1:2], st2[1:-1:2]):
        assert np.array_equal(_bits(a[ok]), _bits(b[ok]))               # (c of every layer)


@pytest.mark.parametrize('name', [c.name for c in CASES])
def test_the_pick_on_a_tie_model_equals_the_oracle_in_every_form(name):
    """Arithmetic 0: the per-step kernels and the persistent decoder, each as the batch, every line alone and the batch reversed --
    the batch against the oracle, all six bit for bit with each other; both modes."""
    case = BY_NAME[name]
    e = _expected(case)
    idx, enc, B = e['idx'], e['enc'], case.B
    every = list(range(B))
    eng = _engine(case, 0)
    got = {}
    try:
        _preconditions(eng, case, idx, enc)
        for persistent in (0, 1):
            eng.set_option('persistent', persistent)
            for mode in MODES:
                _install(eng, case, idx, enc, every)
                got[persistent, mode, 'batch'] = _decode(eng, case, mode)
                parts = []
                for j in every:
                    _install(eng, case, idx, enc, [j])
                    parts.append(_decode(eng, case, mode))
                got[persistent, mode, 'alone'] = _rows_of(parts)
                _install(eng, case, idx, enc, every[::-1])
                got[persistent, mode, 'reversed'] = _reordered(_decode(eng, case, mode), every[::-1])
        eng.set_option('persistent', -1)
    finally:
        eng.close()
    for mode in MODES:
        _against_the_oracle(case, got[0, mode, 'batch'], e['want'][mode], mode, every, 'per step')
        _against_the_oracle(case, got[1, mode, 'batch'], e['want'][mode], mode, every, 'persistent (%s)' % greedy_form(case.V))
        for persistent in (0, 1):
            for what in ('alone', 'reversed'):
                _same_bits(got[persistent, mode, 'batch'], got[persistent, mode, what], mode, (persistent, what))
        _same_bits(got[0, mode, 'batch'], got[1, mode, 'batch'], mode, 'persistent against per step')


@pytest.mark.parametrize('name', [c.name for c in CASES])
def test_the_pick_on_a_tie_model_under_the_split_arithmetic(name):
    """Arithmetic 2 (bf16x3-split operands; greedy decodes step kernel by kernel there): `persistent` 0 against the oracle."""
    case = BY_NAME[name]
    e = _expected(case)
    every = list(range(case.B))
    eng = _engine(case, 2)
    got = {}
    try:
        _preconditions(eng, case, e['idx'], e['enc'])
        eng.set_option('persistent', 0)
        for mode in MODES:
            _install(eng, case, e['idx'], e['enc'], every)
            got[mode] = _decode(eng, case, mode)
    finally:
        eng.close()
    for mode in MODES:
        _against_the_oracle(case, got[mode], e['want'][mode], mode, every, 'split arithmetic')


@pytest.mark.parametrize('name', [c.name for c in CASES if c.nan_row is not None])
@pytest.mark.parametrize('persistent', (0, 1))
def test_a_nan_row_leaves_the_other_rows_their_bits(name, persistent):
    """Mode 0: the NaN row reports index 1 and a NaN probability at every step and the call returns OK (fmaxf drops NaN: the row's
    maximum must not hide it); mode 1: CASV_ERR_NAN, the row's length is 1.  Every other row keeps the bits it has in the same batch
    with that row finite."""
    import cor_asv_ann_amd._native as nv
    case = BY_NAME[name]
    e = _expected(case)
    clean_enc = case.encoder_outputs(e['m'], nan_row=None)
    r, every = case.nan_row, list(range(case.B))
    others = [j for j in every if j != r]
    eng = _engine(case, 0)
    got = {}
    try:
        eng.set_option('persistent', persistent)
        for mode in MODES:
            for what, enc in (('nan', e['enc']), ('clean', clean_enc)):
                _install(eng, case, e['idx'], enc, every)
                got[mode, what] = _decode(eng, case, mode)
        eng.set_option('persistent', -1)
    finally:
        eng.close()
    d = got[0, 'nan']
    assert d['rc'] == 0 and (d['len'] == case.S).all() and (d['idx'][r] == 1).all() and np.isnan(d['prob'][r]).all()
    d = got[1, 'nan']
    assert d['rc'] == nv.CASV_ERR_NAN and d['len'][r] == 1 and d['idx'][r, 0] == 1 and np.isnan(d['prob'][r, 0])
    for mode in MODES:
        assert got[mode, 'clean']['rc'] == 0 and np.isfinite(got[mode, 'clean']['prob'][:, 0]).all()
        a, b = _reordered(got[mode, 'nan'], others), _reordered(got[mode, 'clean'], others)
        a['rc'] = b['rc'] = 0
        _same_bits(a, b, mode, 'beside the NaN row')


@pytest.mark.parametrize('V', (40, 256, 640))
def test_persistent_1_runs_the_persistent_decoder(V):
    """Otherwise the forms compared above are not the ones named: with `persistent` = 1 a greedy decode is ONE launch of the profile
    class "persist" (the encoder outputs are handed in, so no encoder launch is counted), with 0 it is none."""
    case = BY_NAME['x_v%d_b37' % V]
    e = _expected(case)
    assert greedy_form(V) == {40: 'quarter', 256: 'quarter_full', 640: 'wave'}[V]
    eng = _engine(case, 0)
    try:
        eng.profile(True)
        counts = []
        for persistent in (1, 0):
            eng.set_option('persistent', persistent)
            for mode in MODES:
                _install(eng, case, e['idx'], e['enc'], list(range(case.B)))
                before = eng.profile_read('persist')['launches']
                assert _decode(eng, case, mode)['rc'] == 0
                counts.append(eng.profile_read('persist')['launches'] - before)
        eng.profile(False)
    finally:
        eng.close()
    assert counts == [1, 1, 0, 0], counts
