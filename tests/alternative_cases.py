"""Cases and references of `score_alternatives` (csrc/train_kernels.hip: score_alternatives_kernel; csrc/score.hip:
casv_score_get_alternatives) -- helpers, no test.  The head table, the model table, the oracles and the units are tests/score_cases.py's.

  alts64 / alts32      the definition restated row by row: indices from the float32 logits (exact), log-probabilities and entropy
                       in float64, and in float32 numpy with the head's formula
  head_ks              the head table (HEAD_V x HEAD_SCALES, 64 rows each) with K in {1, 2, 5, min(V, 64)}
  constructed_rows     [(name, x, K)]: score_cases' rows and the rows built for the order, the K-th boundary and the -inf members
  e_h                  the float32 reference's own entropy error over the head table, in units of UNIT * (|H64| + 1)
  compare              the GPU test's comparator of the kernel alone: (indices exact, logp excess, entropy excess)
  MISTAKES             six wrong heads the comparator must catch (tests/test_alternative_cases.py)
  model_refs           per model case and K: the fp64 and fp32 oracles' sorted lists, the near ties, the fp64 entropy
"""
import functools

import numpy as np

from tests import score_cases as sc


# ------------------------------------------------------------------------------------------------------------------ the definition
def _order(row):
    """The total order: x descending as floats (-0.0 == +0.0), the lower index first among equals."""
    return np.argsort(-row, kind='stable')


def _alts(x, K, dt, order=_order, mask_inf=True):
    x = np.asarray(x, np.float32)
    R, V = x.shape
    assert 1 <= K <= min(V, 64)
    idx = np.full((R, K), -1, np.int32)
    logp = np.full((R, K), np.nan, dt)
    ent = np.full(R, np.nan, dt)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for r in range(R):
            row = x[r].astype(dt)
            if np.isnan(row).any() or not np.isfinite(np.max(row)):
                continue
            m = np.max(row)
            first = order(x[r])[:K]
            d = row - m
            e = np.exp(d)
            s = np.sum(e, dtype=dt)
            idx[r] = first
            logp[r] = (row[first] - m) - np.log(s)
            keep = row > -np.inf if mask_inf else np.ones(V, bool)
            ent[r] = np.log(s) - np.sum(e[keep] * d[keep], dtype=dt) / s
    return idx, logp, ent


def alts64(x, K):
    return _alts(x, K, np.float64)


def alts32(x, K):
    return _alts(x, K, np.float32)


# ------------------------------------------------------------------------------------------------------------------ the tables
def head_ks(V):
    return sorted({k for k in (1, 2, 5, min(V, 64)) if k <= V})


def constructed_rows():
    """[(name, x (V,), K)]: score_cases.constructed_rows() with K = 5, and the rows built for this kernel.  In every `boundary_*` row
    a group of equal entries is larger than the places left for it: the lower indices must win."""
    rng = np.random.default_rng(11)
    rows = [(name, x, 5) for name, x, _ in sc.constructed_rows()]

    def base(V, lo=-3.0, hi=-1.0):
        return rng.uniform(lo, hi, V).astype(np.float32)
    # (V, entries above the group, the group's indices -- across lanes and across a lane's passes --, K)
    for V, above, group, K in ((40, (20,), (38, 3, 31, 9), 3), (96, (50,), (69, 5, 70, 20), 3),
                               (257, (100,), (256, 0, 64, 128, 192), 4), (640, (300, 7), (69, 581, 133, 5, 639), 5),
                               (640, (), (581, 69, 5), 2)):
        x = base(V)
        for i, a in enumerate(above):
            x[a] = 4.0 - i
        x[list(group)] = 2.0
        rows.append(('boundary_%d_k%d_%s' % (V, K, '_'.join(map(str, group))), x, K))
    x = base(40)
    x[[4, 30]] = 0.0
    x[[2, 9, 35]] = -0.0
    rows.append(('mixed_zeros', x, 4))
    x = base(40, 1.0, 2.0)                  # zeros BELOW the rest: they close the list
    x[[4, 30]] = 0.0
    x[[2, 9, 35]] = -0.0
    rows.append(('mixed_zeros_last', x, 38))
    x = np.full(40, -np.inf, np.float32)
    x[[7, 12, 33, 39]] = (-1.5, 0.25, -1.5, -4.0)
    rows.append(('minus_inf_members', x, 8))
    rows.append(('v2_k2', np.array([-0.5, 1.25], np.float32), 2))
    rows.append(('v2_k2_tied', np.array([0.75, 0.75], np.float32), 2))
    rows.append(('v4096_k64', (rng.standard_normal(4096) * 3).astype(np.float32), 64))
    x = (rng.standard_normal(4096) * 3).astype(np.float32)
    x[[4095, 64, 2048, 1, 4032]] = 20.0
    rows.append(('v4096_k3_tied', x, 3))
    return rows


# ------------------------------------------------------------------------------------------------------------------ the bounds
@functools.lru_cache(maxsize=None)
def e_h():
    """The float32-numpy reference's largest entropy error over the head table, in units: computed, not assumed."""
    worst = 0.0
    for V in sc.HEAD_V:
        for s in sc.HEAD_SCALES:
            x, _ = sc.head_case(V, s)
            worst = max(worst, float(sc.units(alts32(x, 1)[2], alts64(x, 1)[2]).max()))
    return worst


def compare(got, x, K, want=None):
    """The GPU test's checks of the kernel alone on rows x (R,V): (alt_idx exact against alts64, largest alt_logp error over its bound
    of 4 e_np() units, largest entropy error over its bound of 4 e_h() units); inf where a NaN / -inf is not where it belongs."""
    idx, lp, h = want or alts64(x, K)
    return (np.array_equal(got[0], idx), float(sc.units_or_inf(got[1], lp).max(initial=0.0)) / (4 * sc.e_np()),
            float(sc.units_or_inf(got[2], h).max(initial=0.0)) / (4 * e_h()))


# ------------------------------------------------------------------------------------------------------------------ six wrong heads
# name -> (x (R,V), K, pad_value) -> (alt_idx, alt_logp, entropy) in float32
def _padding_read(x, K, pad):
    V = x.shape[1]
    xp = np.full((x.shape[0], (V + 31) // 32 * 32), pad, np.float32)
    xp[:, :V] = x
    return alts32(xp, K)


def _higher_index_first(x, K, pad):
    return _alts(x, K, np.float32, order=lambda row: len(row) - 1 - np.argsort(-row[::-1], kind='stable'))


def _minus_zero_below(x, K, pad):
    return _alts(x, K, np.float32, order=lambda row: np.lexsort((np.arange(len(row)), np.signbit(row) & (row == 0), -row)))


def _kth_is_the_next(x, K, pad):
    def order(row):
        o = _order(row)
        return np.concatenate([o[:K - 1], o[K:]]) if len(row) > K else o
    return _alts(x, K, np.float32, order=order)


def _tied_entry_twice(x, K, pad):
    def order(row):
        o = _order(row).copy()
        for j in range(1, len(o)):
            if row[o[j]] == row[o[j - 1]]:
                o[j] = o[j - 1]
        return o
    return _alts(x, K, np.float32, order=order)


def _entropy_nan_with_minus_inf(x, K, pad):
    return _alts(x, K, np.float32, mask_inf=False)


MISTAKES = {'padding_column_read': _padding_read, 'higher_index_first': _higher_index_first, 'minus_zero_below_plus_zero': _minus_zero_below,
            'kth_place_takes_the_next': _kth_is_the_next, 'tied_entry_twice': _tied_entry_twice,
            'entropy_nan_with_minus_inf': _entropy_nan_with_minus_inf}


# ------------------------------------------------------------------------------------------------------------------ the model
def tol(p):
    """The logp bound of tests/test_gpu_score.py around a probability p."""
    with np.errstate(divide='ignore'):
        return 2e-4 + 2e-6 / p


def sorted_lists(P, n):
    """The first n entries of every position of probabilities P (B,U,V) in the kernel's order: (indices, log-probabilities)."""
    with np.errstate(divide='ignore'):
        lp = np.log(P.astype(np.float64))
    order = np.argsort(-P, axis=2, kind='stable')[:, :, :n]
    return order.astype(np.int32), np.take_along_axis(lp, order, axis=2), lp


def refs_of(o, K):
    """From a case's oracles (score_cases.oracles / candidate_cases.oracles): idx64 / lps64 the fp64 oracle's first K + 1 entries
    and their log-probabilities, idx32 the fp32 oracle's, lp64 (B,U,V) all log-probabilities, near (B,U) the positions with a near
    tie among the first K + 1 -- a gap of consecutive log-probabilities not above tol(p_j) + tol(p_j+1) --, H64 the entropy."""
    n = min(K + 1, o['P64'].shape[2])
    idx64, lps64, lp64 = sorted_lists(o['P64'], n)
    idx32 = sorted_lists(o['P32'], n)[0]
    p = np.exp(lps64)
    near = ((lps64[:, :, :-1] - lps64[:, :, 1:]) <= tol(p[:, :, :-1]) + tol(p[:, :, 1:])).any(axis=2)
    P = o['P64'].astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        H64 = -np.where(P > 0, P * np.log(P), 0.0).sum(axis=2)
    return dict(idx64=idx64, lps64=lps64, idx32=idx32, lp64=lp64, near=near, H64=H64)


@functools.lru_cache(maxsize=None)
def model_refs(c, K):
    return refs_of(sc.oracles(c), K)


def check_model(alt_idx, alt_logp, entropy, ref, K):
    """The GPU test's checks of a model's alternatives (rows, U, K) against the fp64 oracle: the lists where no near tie is, the
    order-statistic bounds and the entropy everywhere.  Returns the figures it asserted on."""
    idx64, lps64, lp64, near, H64 = ref['idx64'][:, :, :K], ref['lps64'][:, :, :K], ref['lp64'], ref['near'], ref['H64']
    assert alt_idx.shape == idx64.shape == alt_logp.shape and entropy.shape == H64.shape
    assert np.array_equal(alt_idx[~near], idx64[~near])
    srt = np.sort(alt_idx, axis=2)
    assert (srt[:, :, 1:] != srt[:, :, :-1]).all() and (alt_idx >= 0).all() and (alt_idx < lp64.shape[2]).all()
    t = tol(np.exp(lps64))
    worst_lp = float((np.abs(alt_logp - lps64) / t).max())
    picked = np.take_along_axis(lp64, alt_idx.astype(np.int64), axis=2)
    worst_pick = float(((lps64 - picked) / (2 * t)).max())
    worst_h = float((np.abs(entropy - H64) / tol(np.exp(-H64))).max())
    print('K=%d: alt_logp %.3f, the picked index %.3f, entropy %.3f of the bounds; %d of %d positions near a tie'
          % (K, worst_lp, worst_pick, worst_h, int(near.sum()), near.size))
    assert worst_lp <= 1 and worst_pick <= 1 and worst_h <= 1
    return worst_lp, worst_pick, worst_h
