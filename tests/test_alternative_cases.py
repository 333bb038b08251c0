"""The references and bounds of tests/test_gpu_score_alternatives.py hold on the CPU: the float32 and float64 restatements agree on
the exact outputs and with the scoring head's log-probabilities, the float32 entropy's own error is computed, the comparator catches
six wrong heads, the model cases are far enough from ties for the order-statistic bounds, and the facade's score_alternatives and
alternatives_to_confmat do their bookkeeping on a stub engine."""
import numpy as np
import pytest

from tests import alternative_cases as ac
from tests import score_cases as sc


def _bits(a):
    return np.asarray(a, np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------ 1. the definition, twice
def _agree(x, K, name):
    a, b = ac.alts32(x, K), ac.alts64(x, K)
    assert np.array_equal(a[0], b[0]), name
    R, V = x.shape
    for r in range(R):                      # alt_logp: the bits of the head's logp for that index as target
        if a[0][r, 0] < 0:
            assert np.isnan(a[1][r]).all() and np.isnan(a[2][r]) and (a[0][r] == -1).all(), name
            assert np.isnan(sc.head32(x[r:r + 1], [0])[0][0]), name
            continue
        for j in range(K):
            want = sc.head32(x[r:r + 1], [a[0][r, j]])[0]
            assert np.array_equal(_bits(a[1][r, j:j + 1]), _bits(want)), (name, r, j)
    return a, b


@pytest.mark.parametrize('V', sc.HEAD_V)
def test_both_restatements_agree_on_the_head_table(V):
    for s in sc.HEAD_SCALES:
        x, _ = sc.head_case(V, s)
        for K in ac.head_ks(V):
            a, b = _agree(x[:8] if V == 4096 and K == 64 else x, K, (V, s, K))          # (the head32 loop is the slow part)
            assert (np.diff(b[1], axis=1) <= 0).all()                                    # most probable first
    assert ac.head_ks(2) == [1, 2] and ac.head_ks(63) == [1, 2, 5, 63] and ac.head_ks(4096) == [1, 2, 5, 64]


def test_constructed_rows_say_what_their_names_say():
    rows = {}
    for name, x, K in ac.constructed_rows():
        a, b = _agree(x[None], K, name)
        rows[name] = (b[0][0], b[1][0], b[2][0], x, K)
    idx, lp, h, x, K = rows['all_equal']
    assert idx.tolist() == [0, 1, 2, 3, 4] and np.allclose(lp, -np.log(40)) and abs(h - np.log(40)) < 1e-12
    seen = set()
    for name, (idx, lp, h, x, K) in rows.items():
        if name.startswith('boundary_'):
            V, group = int(name.split('_')[1]), [int(v) for v in name.split('_')[3:]]
            above = K - int((x > 2.0).sum())
            assert 0 < above < len(group) and idx[K - above:].tolist() == sorted(group)[:above], name     # the lower indices win
            assert len({g % 64 for g in group}) > 1 or len({g // 64 for g in group}) > 1      # across lanes, or across a lane's passes
            seen.add(V)
        if name.startswith('nan_at') or name in ('plus_inf', 'all_minus_inf'):
            assert (idx == -1).all() and np.isnan(lp).all() and np.isnan(h), name
    assert seen == {40, 96, 257, 640}
    assert {'nan_at_0_of_40', 'nan_at_17_of_40', 'nan_at_39_of_40', 'nan_at_256_of_257'} <= set(rows)
    idx, lp, h, x, K = rows['mixed_zeros']
    assert idx.tolist() == [2, 4, 9, 30] and len(set(lp.tolist())) == 1              # index order through both signs of zero
    idx, lp, h, x, K = rows['mixed_zeros_last']
    assert idx[-3:].tolist() == [2, 4, 9]
    idx, lp, h, x, K = rows['minus_inf_members']
    assert idx.tolist() == [12, 7, 33, 39, 0, 1, 2, 3] and (lp[4:] == -np.inf).all() and np.isfinite(lp[:4]).all() and np.isfinite(h)
    idx, lp, h, x, K = rows['minus_inf_at_target']
    assert np.isfinite(h) and 6 not in idx.tolist()
    assert rows['v2_k2'][0].tolist() == [1, 0] and rows['v2_k2_tied'][0].tolist() == [0, 1]
    assert rows['v4096_k64'][4] == 64 and len(rows['v4096_k64'][3]) == 4096
    assert rows['v4096_k3_tied'][0].tolist() == [1, 64, 2048]


# ------------------------------------------------------------------------------------------------ 2. the entropy's own float32 error
def test_float32_entropy_error_in_units():
    e = ac.e_h()
    print('E_H = %.3f units of 2^-24 (|H64| + 1); E_np = %.3f' % (e, sc.e_np()))
    assert 0 < e <= 8
    x, _ = sc.head_case(4096, 1.0)
    assert ac.alts64(x, 1)[2].min() > 7             # (near log V at scale 1 ...)
    x, _ = sc.head_case(4096, 80.0)
    assert ac.alts64(x, 1)[2].min() < 1e-3          # (... and next to nothing at scale 80)


# ------------------------------------------------------------------------------------------------ 3. the comparator can fail
def test_six_mistakes_are_caught():
    named = {name: (x[None], K) for name, x, K in ac.constructed_rows()}
    M = ac.MISTAKES
    # a padding column read: negative logits, padding 0 -- the padding columns lead the list; padding NaN -- the row is invalid
    x, K = named['negative_only']
    ok, lp, h = ac.compare(M['padding_column_read'](x, K, 0.0), x, K)
    assert not ok and lp >= 10 and h >= 10
    ok, lp, h = ac.compare(M['padding_column_read'](x, K, np.nan), x, K)
    assert not ok and lp == np.inf and h == np.inf
    # the higher index first: every row whose group does not fit
    for name in ('all_equal', 'boundary_40_k3_38_3_31_9', 'boundary_96_k3_69_5_70_20', 'boundary_257_k4_256_0_64_128_192',
                 'boundary_640_k5_69_581_133_5_639', 'boundary_640_k2_581_69_5', 'v4096_k3_tied', 'v2_k2_tied'):
        x, K = named[name]
        ok, lp, h = ac.compare(M['higher_index_first'](x, K, 0.0), x, K)
        assert not ok and lp <= 1 and h <= 1, name
    # -0.0 below +0.0
    for name in ('mixed_zeros', 'mixed_zeros_last'):
        x, K = named[name]
        ok, lp, h = ac.compare(M['minus_zero_below_plus_zero'](x, K, 0.0), x, K)
        assert not ok and lp <= 1 and h <= 1, name
    # the K-th place taken by the (K+1)-th entry: an exact output flips on rows with and without ties
    for name in ('negative_only', 'boundary_40_k3_38_3_31_9', 'minus_inf_members', 'v4096_k64'):
        x, K = named[name]
        assert not ac.compare(M['kth_place_takes_the_next'](x, K, 0.0), x, K)[0], name
    x, _ = sc.head_case(257, 10.0)
    ok, lp, h = ac.compare(M['kth_place_takes_the_next'](x, 5, 0.0), x, 5)
    assert not ok and lp >= 10
    # a tied entry listed twice
    for name in ('all_equal', 'boundary_96_k3_69_5_70_20', 'mixed_zeros', 'minus_inf_members', 'v2_k2_tied'):
        x, K = named[name]
        ok, lp, h = ac.compare(M['tied_entry_twice'](x, K, 0.0), x, K)
        assert not ok and lp <= 1, name
    # the entropy NaN on a row with an -inf entry
    for name in ('minus_inf_at_target', 'minus_inf_members'):
        x, K = named[name]
        ok, lp, h = ac.compare(M['entropy_nan_with_minus_inf'](x, K, 0.0), x, K)
        assert ok and lp <= 1 and h == np.inf, name
    # ... and the right head passes all of them
    for x, K in list(named.values()) + [(sc.head_case(257, 10.0)[0], 5), (sc.head_case(640, 80.0)[0], 64)]:
        ok, lp, h = ac.compare(ac.alts32(x, K), x, K)
        assert ok and lp <= 1 and h <= 1


# ------------------------------------------------------------------------------------------------ 4. the model cases' condition
@pytest.mark.parametrize('c', sc.MODEL_CASES, ids=sc.IDS)
def test_model_cases_are_far_enough_from_ties(c):
    """What the GPU test's order-statistic bounds rest on: both oracles list the same K indices at every position, near ties among
    the first K + 1 entries are rare, and the K-th entry is probable enough for its bound to separate it from the tail."""
    for K in (4, 8):
        ref = ac.model_refs(c, K)
        assert np.array_equal(ref['idx32'][:, :, :K], ref['idx64'][:, :, :K])
        share = ref['near'].mean()
        kth = float(np.exp(ref['lps64'][:, :, K - 1]).min())
        print('%s K=%d: %d of %d positions near a tie, smallest p of the K-th entry %.2e' % (sc.case_id(c), K, ref['near'].sum(), ref['near'].size, kth))
        assert share <= 1 / 8
        assert kth >= 1e-3
        assert np.allclose(ref['H64'], -(np.exp(ref['lp64']) * ref['lp64']).sum(axis=2), atol=1e-12)


# ------------------------------------------------------------------------------------------------ 5. the facade on a stub engine
class _StubEngine(object):
    """score_targets / score_alternatives with made-up values that encode (call, row, position, place), and a record of the calls."""
    def __init__(self, voc_size):
        self.calls, self.ks, self.V = [], [], voc_size

    def score_targets(self, idx, val, dec_in, dec_out, want_align=False):
        B, U = dec_out.shape
        self.calls.append((idx.copy(), dec_in.copy(), dec_out.copy(), want_align))
        self.shape = (B, U)
        count = (dec_out >= 0).sum(axis=1).astype(np.int32)
        z = np.zeros((B, U), np.float32)
        return z, z.astype(np.int32), z.astype(np.int32), np.zeros(B), count, None

    def score_alternatives(self, K, want_entropy=True):
        assert 1 <= K <= min(self.V, 64)
        B, U = self.shape
        k = len(self.calls) - 1
        self.ks.append(K)
        dec_out = self.calls[-1][2]
        alt_idx = np.empty((B, U, K), np.int32)
        alt_idx[:, :, 0] = np.where(dec_out >= 0, dec_out, 3)           # the target first,
        if K > 1:
            alt_idx[:, :, 1] = 0                                        # then index 0: no character,
        for j in range(2, K):
            alt_idx[:, :, j] = 10 + j                                   # then fixed others
        if k == 0:
            alt_idx[0, 0, :] = -1                                       # an invalid row
        alt_logp = -(100.0 * k + 10.0 * np.arange(B)[:, None, None] + np.arange(U)[None, :, None] + 0.125 * np.arange(K)[None, None, :])
        entropy = (100.0 * k + 10.0 * np.arange(B)[:, None] + np.arange(U)[None, :]).astype(np.float32)
        return alt_idx, alt_logp.astype(np.float32), entropy if want_entropy else None


def _stub_facade(batch_size, voc_size=100):
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence
    from oracle import make_vocabulary
    s2s = Sequence2Sequence()
    s2s.depth, s2s.width, s2s.batch_size = 1, 32, batch_size
    s2s.mapping, s2s.voc_size = make_vocabulary(voc_size), voc_size
    s2s.engine = _StubEngine(voc_size)
    s2s._require_engine = lambda: s2s.engine
    s2s.status = 2
    return s2s


SOURCES = ['abc\n', 'de\n', 'fgh\n', '', 'ij\n']
TARGETS = ['abd\n', '', 'fg\n', 'xy\n', 'ijkl\n']


def test_score_alternatives_bookkeeping_on_a_stub_engine():
    s2s = _stub_facade(2)
    alts, ents = s2s.score_alternatives(SOURCES, TARGETS, k=4)
    calls = s2s.engine.calls
    lines = _stub_facade(2)
    lines.score_lines(SOURCES, TARGETS)
    assert len(calls) == len(lines.engine.calls) == 2                  # the chunks of score_lines: pairs 0, 2 | 4
    for mine, theirs in zip(calls, lines.engine.calls):
        assert all(np.array_equal(a, b) for a, b in zip(mine[:3], theirs[:3])) and mine[3] is False
    assert s2s.engine.ks == [4, 4]
    for j in (1, 3):                                                    # skipped as score_lines skips them
        assert alts[j] == [] and ents[j] == []
    assert [len(a) for a in alts] == [4, 0, 3, 0, 5] == [len(e) for e in ents]
    assert alts[0][0] == []                                             # the invalid row: no alternative (its entropy stays)
    c_i, i_c = s2s.mapping
    for j, (k, i) in ((0, (0, 0)), (2, (0, 1)), (4, (1, 0))):
        for u, position in enumerate(alts[j]):
            if (j, u) == (0, 0):
                continue
            assert len(position) == 3                                   # index 0 is left out
            assert [ch for ch, _ in position] == [TARGETS[j][u], i_c[12], i_c[13]]
            assert [lp for _, lp in position] == [-(100.0 * k + 10.0 * i + u + 0.125 * place) for place in (0, 2, 3)]
            assert all(isinstance(ch, str) and isinstance(lp, float) for ch, lp in position)
        assert ents[j] == [100.0 * k + 10.0 * i + u for u in range(len(TARGETS[j]))] and all(isinstance(e, float) for e in ents[j])
    assert '' not in [ch for line in alts for position in line for ch, _ in position]
    s2s = _stub_facade(2, voc_size=6)                                   # k above the vocabulary: the call uses voc_size
    s2s.score_alternatives(['ab\n'], ['ab\n'], k=9)
    assert s2s.engine.ks == [6]
    assert s2s.score_alternatives([], []) == ([], [])
    s2s.status = 1
    with pytest.raises(AssertionError):
        s2s.score_alternatives(SOURCES, TARGETS)


def test_alternatives_to_confmat_feeds_correct_lines_input():
    from cor_asv_ann_amd.seq2seq import alternatives_to_confmat
    s2s = _stub_facade(8)
    k = 4
    alts, _ = s2s.score_alternatives(SOURCES, TARGETS, k=k)
    live = [j for j in range(len(SOURCES)) if alts[j]]
    # made-up log-probabilities in [-3, 0]: the stub's are too small to tell a floor from nothing
    rng = np.random.default_rng(3)
    alts = [[sorted(((ch, -float(rng.uniform(0, 3))) for ch, _ in pos), key=lambda t: -t[1]) for pos in line] for line in alts]
    conf = [alternatives_to_confmat(alts[j]) for j in live]
    for j, line in zip(live, conf):
        kept = [pos for pos in alts[j] if pos]
        assert len(line) == len(kept)
        for chunk, pos in zip(line, kept):
            assert [ch for ch, _ in chunk] == [ch for ch, _ in pos] and [p for _, p in chunk] == [np.exp(lp) for _, lp in pos]
    idx, val, _ = s2s._sparse_lines([TARGETS[j] for j in live], conf)
    B, T, A = idx.shape
    assert B == len(live) and A <= k and T == max(len(line) for line in conf)
    for b, line in enumerate(conf):
        for t, chunk in enumerate(line):
            assert idx[b, t, :len(chunk)].tolist() == [s2s.mapping[0][ch] for ch, _ in chunk]
            assert np.array_equal(val[b, t, :len(chunk)], np.array([p for _, p in chunk], np.float32))
        assert (idx[b, len(line):] == -1).all()
    # the floor drops the improbable, never the first of a position
    for floor in (0.3, 0.9, 2.0):
        for j in live:
            full, cut = alternatives_to_confmat(alts[j]), alternatives_to_confmat(alts[j], floor=floor)
            assert len(cut) == len(full)
            for a, b in zip(full, cut):
                assert b and b[0] == a[0] and b[1:] == [(ch, p) for ch, p in a[1:] if p >= floor]
    assert all(len(chunk) == 1 for j in live for chunk in alternatives_to_confmat(alts[j], floor=2.0))
    assert alternatives_to_confmat([]) == []


def test_both_entries_are_bound():
    from cor_asv_ann_amd import _native as nv
    assert len(nv.SIGNATURES['casv_score_get_alternatives'][1]) == 5
    assert len(nv.SIGNATURES['casv_debug_alternatives_rows'][1]) == 9
