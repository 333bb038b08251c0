"""The train step's weight-gradient contraction C[m][n] (+)= sum_k A[k][m] * B[k][n] (csrc/gemm_tn.hip, gemm_tn_split.hip) on the host:
the shapes its call sites use (csrc/train.hip, run_gemm_tn), a mirror of the launch plan (K shares), and a float64 reference with
errors in rounding units.  Shared by tests/test_gpu_gemm_tn.py (device against float64) and tests/test_gemm_tn_bounds.py (the
bounds' power to see a dropped or doubled K range, without a GPU)."""
import numpy as np

# tests/test_gpu_gemm.py's units and bounds: error / (2^-24 * (sum_k |a||b| + |C_in|)); a missing or doubled K tile shows as 1e3 and more
RMS_BOUND, MAX_BOUND = 1.5, 12.0
TK = 16                 # k-tile of both kernels


def _pad32(x):
    return (x + 31) // 32 * 32


def plan(M, N, K, split_arith, ordered, ncu=256):
    """(split, shares, nonempty) of a launch: launch_gemm_tn_any's choice under the train step's arithmetic (split_arith: 2 or 0).
    The ordered form plans for 256 CUs whatever the device has (gemm_tn_split_shares, tn_ordered_plan), the atomic form for ncu."""
    split, ks = False, 1
    if split_arith and M % 256 == 0 and N % 256 == 0 and K >= 64 * TK and K % TK == 0:
        tiles = (M // 256) * (N // 256)
        cus = 256 if ordered else ncu
        ks = max(1, min(cus // tiles, (K // TK) // 64))
        split = tiles * ks >= (128 if ordered else ncu // 2)
    if split:
        ktiles = K // TK
    else:
        tiles = -(-M // 128) * -(-N // 128)
        ktiles = -(-K // TK)
        ks = max(1, min(-(-512 // tiles), ktiles // 64))
    per = -(-ktiles // ks)
    return int(split), ks, -(-ktiles // per)


def share_ranges(K, split, ks):
    """[k0, k1) of every K share that holds k-tiles, in share (z) order."""
    ktiles = K // TK if split else -(-K // TK)
    per = -(-ktiles // ks)
    return [(z * per * TK, min(K, (z + 1) * per * TK)) for z in range(ks) if z * per < ktiles]


# One row per call-site shape: (name, M, Mstore, N, K, A columns / offset, B columns / offset).  A is a window [K][M] at column
# a_off of an array [K][lda]; B likewise.  Widths are the device's (W padded to 32, V to 32: engine.py, dead units).
def _rows():
    rows = []
    # configs[3]: d4 W512 V256 B512 T = U = 100, C = W (depth > 1, not deep)
    W, B, T = 512, 512, 100
    rows += [('c3_enc1bw_dWr_hprev', 4 * W, 4 * W, W, B * (T - 1), (4 * W, 0), (2 * W, W)),      # hp = H1 + W, ld 2W (train.hip, layer_backward_finish)
             ('c3_E', 256, 256, W, T * B, (256, 0), (W, 0)),                                     # dlog [UB][Vp] . G (train.hip, backward_cell)
             ('c3_att_dWaT', W, W, W, T * B, (W, 0), (2 * W, W)),                                # RecIn + C, ld kr = C + W (:967)
             ('c3_bridge', W, W, W, B, (W, 0), (W, 0))]                                          # K = B (:985)
    # mid size: d2 W256 B512 T64, where the split and the ordered split forms are taken
    W, B, T = 256, 512, 64
    rows += [('mid_enc1_dWx', 4 * W, 4 * W, W, B * T, (4 * W, 0), (W, 0)),
             ('mid_enc1_dWr_hprev', 4 * W, 4 * W, W, B * (T - 1), (4 * W, 0), (2 * W, 0)),
             ('mid_dec_top_dWr', 4 * W, 4 * W, 2 * W, (T + 1) * B, (4 * W, 0), (2 * W, 0)),     # N = kr = C + W
             # (B * U a multiple of 32 k-tiles splits evenly into 32 shares; at B = 400, U = 83 the last share is partly filled)
             ('mid_b400_dec_top_dWr', 4 * W, 4 * W, 2 * W, 400 * 83, (4 * W, 0), (2 * W, 0))]
    # the small train tests (tests/test_gpu_train.py): (W, V, B, L) -> widths padded; T = L + 1, U = L + 2
    for W0, V, B, L, d in ((20, 24, 3, 7, 1), (32, 40, 4, 9, 2), (50, 40, 4, 9, 2), (64, 96, 8, 12, 3), (96, 40, 5, 8, 2),
                           (128, 40, 37, 7, 3), (160, 40, 3, 6, 3), (256, 48, 5, 6, 2)):
        W, Vp = _pad32(W0), _pad32(V)
        C = 2 * W if d == 1 else W
        T, U = L + 1, L + 2
        t = 'w%d_b%d' % (W0, B)
        rows += [(t + '_enc1_dWx', 4 * W, 4 * W, W, B * T, (4 * W, 0), (W, 0)),                    # N = kx
                 (t + '_enc1_dWr_hprev', 4 * W, 4 * W, W, B * (T - 1), (4 * W, 0), (2 * W, W)),     # N = W, hs window
                 (t + '_dec_top_dWr', 4 * W, 4 * W, W + C, U * B, (4 * W, 0), (W + C, 0)),          # N = kr = W + C
                 (t + '_E', Vp, V, W, U * B, (Vp, 0), (W, 0)),                                      # Mstore = V < Vp
                 (t + '_att_dWaT', W, W, W, U * B, (W, 0), (W + C, C)),
                 (t + '_bridge', W, W, W, B, (W, 0), (W, 0))]
    return rows


ROWS = _rows()
IDS = [r[0] for r in ROWS]


def operands(row):
    """Random A, B windows (views into wider arrays, as the train step passes them), C_in and colsum_in for one table row."""
    name, M, Mstore, N, K, (lda, aoff), (ldb, boff) = row
    rng = np.random.default_rng(sum(map(ord, name)) * 7919 + K)
    Af = rng.standard_normal((K, lda), dtype=np.float32)
    Bf = rng.standard_normal((K, ldb), dtype=np.float32)
    A, B = Af[:, aoff:aoff + M], Bf[:, boff:boff + N]
    c_in = (rng.standard_normal((Mstore, N)) * np.sqrt(K)).astype(np.float32)
    cs_in = (rng.standard_normal(Mstore) * np.sqrt(K)).astype(np.float32)
    return A, B, c_in, cs_in


def reference(A, B, Mstore, chunk=4096):
    """float64 (sum_k A[k][m] B[k][n], sum_k |A[k][m]||B[k][n]|) over m < Mstore, and the column sums (sum, sum of |.|)."""
    K = A.shape[0]
    ref = np.zeros((Mstore, B.shape[1])); mag = np.zeros_like(ref)
    for k0 in range(0, K, chunk):
        a = A[k0:k0 + chunk, :Mstore].astype(np.float64); b = B[k0:k0 + chunk].astype(np.float64)
        ref += a.T @ b
        mag += np.abs(a).T @ np.abs(b)
    a = A[:, :Mstore].astype(np.float64)
    return ref, mag, a.sum(0), np.abs(a).sum(0)


def partial(A, B, Mstore, k0, k1):
    """float64 sum over the K rows [k0, k1) alone."""
    return A[k0:k1, :Mstore].astype(np.float64).T @ B[k0:k1].astype(np.float64)


def errors(got, want, mag):
    """(rms, max) of got - want in units of 2^-24 * mag."""
    e = (np.asarray(got, np.float64) - want) / (mag * 2.0 ** -24)
    return float(np.sqrt(np.mean(e ** 2))), float(np.abs(e).max())
