"""The weight-gradient launcher as the train step calls it (C ABI: casv_debug_contract_tn -> launch_gemm_tn_any, the dispatch that
run_gemm_tn uses), every form against a float64 product on the host.

run_gemm_tn always accumulates, adds the bias gradient as column sums, stores fewer rows than it computes for the tied projection
(Mstore = V < M = Vp), reads column windows of wider buffers and, with the "deterministic" option, takes the ordered form: per-share
partials in a workspace, then tn_reduce_kernel adds them in share order.  The table in tests/tn_reference.py holds the shapes of its
call sites; every row runs under the fp32-input (0) and the bf16x3-split (2) arithmetic, atomic and ordered, with accumulation and
column sums, and the launch's reported plan is checked against a mirror of it (the ordered shares are part of deterministic training's
reproducibility contract).  tests/test_gemm_tn_bounds.py shows, without a GPU, that the bounds see a dropped or doubled K range.
"""
import numpy as np
import pytest

from tests.tn_reference import ROWS, IDS, RMS_BOUND, MAX_BOUND, TK, plan, share_ranges, operands, reference, errors

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def engines():
    from cor_asv_ann_amd.engine import HipEngine
    a, b = HipEngine(1, 32, 8), HipEngine(1, 32, 8)
    try:
        yield a, b
    finally:
        for e in (a, b):
            e.set_option('arithmetic', -1)
            e.close()


def _run(eng, A, B, c_in, cs_in, Mstore, ordered, accumulate=True):
    C, cs = c_in.copy(), None if cs_in is None else cs_in.copy()
    got = eng.debug_contract_tn(A, B, C, Mstore=Mstore, colsum=cs, accumulate=accumulate, ordered=ordered)
    assert np.isfinite(C).all(), 'an element of C was not written'
    return C, cs, got


# what the table reaches, over all rows (test_the_table_reaches_every_form checks it)
_reached = set()


@pytest.mark.parametrize('row', ROWS, ids=IDS)
def test_every_form_equals_float64(engines, row):
    eng, eng2 = engines
    name, M, Mstore, N, K = row[:5]
    A, B, c_in, cs_in = operands(row)
    ref, mag, csref, csmag = reference(A, B, Mstore)
    want, wmag = ref + c_in, mag + np.abs(c_in)
    cswant, csw_mag = csref + cs_in, csmag + np.abs(cs_in)
    ncu = eng.stat('cus')
    for arith in (0, 2):
        eng.set_option('arithmetic', arith); eng2.set_option('arithmetic', arith)
        for ordered in (False, True):
            C, cs, got = _run(eng, A, B, c_in, cs_in, Mstore, ordered)
            assert got == plan(M, N, K, arith, ordered, ncu), (arith, ordered, got)
            split, ks, nz = got
            ranges = share_ranges(K, split, ks)
            _reached.update({('split', split), ('ks>1', ks > 1), ('k_tail', not split and K % TK != 0), ('row_tail', Mstore % 128 != 0),
                             ('partial_share', ks > 1 and ranges[-1][1] - ranges[-1][0] < ranges[0][1] - ranges[0][0])})
            _reached.add(('ordered_split', split) if ordered else ('atomic_split', split))
            rms, mx = errors(C, want, wmag)
            assert rms < RMS_BOUND and mx < MAX_BOUND, (arith, ordered, got, rms, mx)
            rms, mx = errors(cs, cswant, csw_mag)
            assert rms < RMS_BOUND and mx < MAX_BOUND, ('colsum', arith, ordered, got, rms, mx)
            if ordered:         # the ordered form's bits: a function of the operands alone
                C2, cs2, _ = _run(eng, A, B, c_in, cs_in, Mstore, True)
                C3, cs3, _ = _run(eng2, A, B, c_in, cs_in, Mstore, True)
                assert np.array_equal(C, C2) and np.array_equal(C, C3), (arith, 'ordered C differs between calls / handles')
                assert np.array_equal(cs, cs2) and np.array_equal(cs, cs3), (arith, 'ordered colsum differs between calls / handles')
        # C = (no accumulation, no column sums): every element written, the split-K form clears C first
        C, _, _ = _run(eng, A, B, np.full_like(c_in, np.nan), None, Mstore, False, accumulate=False)
        rms, mx = errors(C, ref, mag)
        assert rms < RMS_BOUND and mx < MAX_BOUND, (arith, 'C =', rms, mx)
    eng.set_option('arithmetic', -1); eng2.set_option('arithmetic', -1)


def test_the_table_reaches_every_form():
    """(after the table: pytest runs the tests of a module in order)"""
    assert _reached, 'test_every_form_equals_float64 did not run'
    for form in (('split', 1), ('split', 0), ('ks>1', True), ('ks>1', False), ('k_tail', True), ('row_tail', True),
                 ('partial_share', True), ('ordered_split', 1), ('ordered_split', 0), ('atomic_split', 1)):
        assert form in _reached, form


def _emulation_rows():
    """Rows whose fp32-kernel ordered form has K shares of fewer than 128 k-tiles: a call on one share's K range alone is then a
    ks = 1 launch of the same chain (the plan gives ks = min(.., k-tiles / 64) = 1)."""
    out = []
    for r in ROWS:
        split, ks, nz = plan(r[1], r[3], r[4], 0, True)
        if ks > 1 and max(k1 - k0 for k0, k1 in share_ranges(r[4], split, ks)) < 128 * TK:
            out.append(r)
    return out


@pytest.mark.parametrize('row', _emulation_rows(), ids=lambda r: r[0])
def test_ordered_form_is_its_documented_order(engines, row):
    """arithmetic 0, ordered: C = C_in + (((part[0] + part[1]) + part[2]) + ...) in fp32, and colsum likewise, where part[z] is the
    device's own ks = 1 contraction over share z's K range -- bit for bit (gemm_tn.hip, tn_reduce_kernel)."""
    eng, _ = engines
    name, M, Mstore, N, K = row[:5]
    A, B, c_in, cs_in = operands(row)
    eng.set_option('arithmetic', 0)
    try:
        C, cs, (split, ks, nz) = _run(eng, A, B, c_in, cs_in, Mstore, True)
        assert not split and ks > 1
        s = cs_s = None
        for k0, k1 in share_ranges(K, split, ks):
            part, cpart, got = _run(eng, A[k0:k1], B[k0:k1], np.zeros_like(c_in), np.zeros_like(cs_in), Mstore, False, accumulate=False)
            assert got[1] == 1, got
            s = part if s is None else s + part
            cs_s = cpart if cs_s is None else cs_s + cpart
        assert np.array_equal(C, c_in + s), 'ordered C is not C_in + the shares in z order'
        assert np.array_equal(cs, cs_in + cs_s), 'ordered colsum is not colsum_in + the shares in z order'
    finally:
        eng.set_option('arithmetic', -1)
