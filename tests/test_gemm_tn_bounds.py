"""Without a GPU: the bounds of tests/test_gpu_gemm_tn.py would see the bugs a split-K weight-gradient launch can have.  For every
row of its shape table, a float64 result with one 16-row K tile dropped, with the last K share's rows dropped, or with a K share
counted twice, is at least 8 x MAX_BOUND away from the true product in its units; so is a column sum with one row dropped."""
import numpy as np
import pytest

from tests.tn_reference import ROWS, IDS, MAX_BOUND, TK, plan, share_ranges, operands, reference, partial, errors


@pytest.mark.parametrize('row', ROWS, ids=IDS)
def test_dropped_or_doubled_k_ranges_exceed_the_bound(row):
    name, M, Mstore, N, K = row[:5]
    A, B, c_in, cs_in = operands(row)
    ref, mag, csref, csmag = reference(A, B, Mstore)
    want, wmag = ref + c_in, mag + np.abs(c_in)
    kt = (K - 1) // TK // 2                                 # a k-tile in the middle (the partial last tile when there is one)
    muts = {'k-tile %d dropped' % kt: want - partial(A, B, Mstore, kt * TK, min(K, (kt + 1) * TK))}
    for arith in (0, 2):
        split, ks, _ = plan(M, N, K, arith, True)
        ranges = share_ranges(K, split, ks)
        muts['last share %s dropped (arithmetic %d)' % (ranges[-1], arith)] = want - partial(A, B, Mstore, *ranges[-1])
        muts['share %s doubled (arithmetic %d)' % (ranges[0], arith)] = want + partial(A, B, Mstore, *ranges[0])
    for what, got in muts.items():
        assert errors(got, want, wmag)[1] >= 8 * MAX_BOUND, (name, what)
    k = K // 2
    cs_got = csref + cs_in - A[k, :Mstore].astype(np.float64)
    assert errors(cs_got, csref + cs_in, csmag + np.abs(cs_in))[1] >= 8 * MAX_BOUND, (name, 'colsum row %d dropped' % k)
