"""Attention window membership, bit for bit, at its edges (csrc/row_kernels.h: att_window_of / att_window / att_window_next).

The spec (oracle/model.py): t' = sum_s a_prev[s] * s + 1 accumulated in float64 and rounded ONCE to float32; position s
is in the window iff float32(|t' - float32(s)|) <= float32(window).  The alignment rows below are float32 rows whose float64 position
sum is exact in every summation order and lands on chosen targets: on integers (|t' - s| = 5 exactly), 1-3 float32 ulps either side
of one, just above / below / on a float32 rounding midpoint (t' rounded once from double), off either end of the line, NaN, +-inf and
|t'| >= 1e9.  At T = 65 and 130 the weights sit on several lanes and on positions past 64.  Checked: the row casv_decoder_step writes
(arithmetic 0 and 2), the NaN rows of casv_decoder_step_lm, and every step of casv_decode_greedy (persistent and per-step; dense and
window form) -- step 0 against the spec window of a0, step s against the spec window of the device's own row s - 1."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import ModelConfig, make_weights
from oracle.decode import OracleModel
from oracle.model import decoder_step
from tests.lm_oracle import lm_step

pytestmark = pytest.mark.gpu

WIN = 5
TS = [1, 5, 11, 64, 65, 130]
EXACT = 2.0 ** -36          # every target and weight product below is a multiple of this, magnitude < 2^9: sums exact in double


def spec_window(t64, T):
    """Boolean (T,) window of the spec for a float64 position sum t64 (= t' before rounding)."""
    with np.errstate(invalid='ignore', over='ignore'):
        tp = np.float32(t64)
        return np.abs(tp - np.arange(T, dtype=np.float32)) <= np.float32(WIN)


def spec_window_of_row(a):
    """Spec window of an alignment row as returned by a kernel (float32): its float64 position sum, correctly rounded."""
    a = np.asarray(a, np.float64)
    with np.errstate(invalid='ignore'):
        t = np.nan if np.isnan(a).any() else (float(np.sum(a * np.arange(a.size))) if np.isinf(a).any()
                                               else float(sum(Fraction(x) * s for s, x in enumerate(a.tolist()) if x)))
    return spec_window(t + 1.0, a.size)


def _row_for(t64, T, rng):
    """A float32 row whose exact position sum + 1 is t64 (a multiple of EXACT): a few 'bulk' weights spread over the lanes, the
    remainder in float32 pieces at positions 1, 2, 4."""
    a = np.zeros(T, np.float32)
    fine = [q for q in (1, 2, 4) if q < T]
    free = [s for s in range(T) if s not in fine]
    if T >= 11:
        pos = rng.choice(free, 3, replace=False)
        if T > 64:
            pos[0] = rng.integers(64, T)        # a position past 64 (lane s - 64 or s - 128)
        a[pos] = rng.integers(0, 1 << 23, 3) * 2.0 ** -24
    rem = Fraction(t64) - 1 - sum(Fraction(float(a[s])) * s for s in range(T))
    for q in fine:
        if rem == 0:
            break
        f = np.float32(float(rem / q))
        a[q] = f
        rem -= Fraction(float(f)) * q
    assert rem == 0, (t64, T)
    assert float(sum(Fraction(float(x)) * s for s, x in enumerate(a))) + 1.0 == t64
    return a


def _targets(T):
    """float64 values of t' on and around the window's edges of a line of T positions."""
    out = []
    for n in sorted({-6, -5, -4, 1, 2, 3, 6, T // 2 + 1, T - 1, T, T + 3, T + 4, T + 5}):
        f = np.float32(n)
        up, dn = f, f
        out.append(float(n))
        for _ in range(3):
            up, dn = np.nextafter(up, np.float32(np.inf)), np.nextafter(dn, np.float32(-np.inf))
            out += [float(up), float(dn)]
        for nb in (np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))):
            mid = (float(f) + float(nb)) / 2
            out += [mid, mid + EXACT, mid - EXACT]
    out += [-5.5, -100.0, T + 4.5, T + 50.0, 0.5]
    return out


def window_rows(T, seed=11):
    """(rows (B,T) float32, t64 (B,) float64) -- the constructed rows, plus one-hot, all-zero and non-finite ones."""
    rng = np.random.default_rng(seed + T)
    rows, ts = [], []
    if T >= 5:
        for t in _targets(T):
            rows.append(_row_for(t, T, rng)); ts.append(t)
    for p in range(T):                                          # one-hot: t' = p + 1
        a = np.zeros(T, np.float32); a[p] = 1
        rows.append(a); ts.append(p + 1.0)
    rows.append(np.zeros(T, np.float32)); ts.append(1.0)        # all zero: t' = 1
    for v, s, t in [(np.nan, 0, np.nan), (np.inf, T - 1, np.inf if T > 1 else np.nan), (-np.inf, T - 1, -np.inf if T > 1 else np.nan),
                    (2e9, T - 1, 2e9 * (T - 1) + 1), (1e9, T - 1, 1e9 * (T - 1) + 1), (3e38, T - 1, 3e38 * (T - 1) + 1)]:
        a = np.zeros(T, np.float32); a[s] = v
        rows.append(a); ts.append(t)
    return np.stack(rows), np.array(ts)


def _setup(T, rows, arithmetic=0):
    from cor_asv_ann_amd.engine import HipEngine
    cfg = ModelConfig(depth=2, width=64, voc_size=40)
    w = make_weights(cfg, emb_scale=4.0)
    B = rows.shape[0]
    rng = np.random.default_rng(5)
    enc = (rng.normal(size=(B, T, cfg.ctx_width)) * 0.5).astype(np.float32)
    states = [(rng.normal(size=(B, cfg.width)) * 0.5).astype(np.float32) for _ in range(2 * cfg.depth)]
    eng = HipEngine(cfg.depth, cfg.width, cfg.voc_size)
    eng.set_weights(w)
    eng.set_option('arithmetic', arithmetic)
    eng.set_encoder_outputs(enc, states, a0=rows)
    return cfg, w, eng, enc, states


def _support_ok(a, want):
    """The row's non-zero support equals the window `want`; an empty window gives an all-NaN row, any other no NaN."""
    if not want.any():
        return bool(np.isnan(a).all())
    return not np.isnan(a).any() and np.array_equal(a != 0, want)


@pytest.mark.parametrize('T', TS)
def test_window_rows_have_exact_position_sums(T):
    rows, ts = window_rows(T)
    for a, t in zip(rows, ts):
        if np.isfinite(a).all() and np.abs(a).max() < 1e8:
            assert np.array_equal(spec_window_of_row(a), spec_window(t, T))


@pytest.mark.parametrize('arithmetic', [0, 2])
@pytest.mark.parametrize('T', TS)
def test_decoder_step_window_is_the_spec_window(T, arithmetic):
    rows, ts = window_rows(T)
    cfg, w, eng, enc, states = _setup(T, rows, arithmetic)
    try:
        B, V = rows.shape[0], cfg.voc_size
        line = np.arange(B, dtype=np.int32)
        p_in = np.random.default_rng(2).dirichlet(np.ones(V), B).astype(np.float32)
        probs, st = eng.decoder_step(line, p_in, states, rows)
        want_p, want_st = decoder_step(cfg, w, p_in, enc, states + [rows])
        for j in range(B):
            assert _support_ok(st[-1][j], spec_window(ts[j], T)), (j, ts[j])
        d = cfg.depth
        assert np.array_equal(np.isnan(probs), np.isnan(want_p))
        for n in range(2 * d):
            assert np.array_equal(np.isnan(st[n]), np.isnan(want_st[n])), n
        if arithmetic == 0:
            probs2, lm, st2 = eng.decoder_step_lm(line, p_in, states, rows)
            assert probs2.tobytes() == probs.tobytes()
            want_lm = lm_step(OracleModel(cfg, w), p_in, enc, states + [rows])
            assert np.array_equal(np.isnan(lm), np.isnan(want_lm))
            assert np.array_equal(np.isnan(lm).all(axis=1), ~np.array([spec_window(t, T).any() for t in ts]))
    finally:
        eng.close()


@pytest.mark.parametrize('persistent', [1, 0])
@pytest.mark.parametrize('T', TS)
def test_greedy_windows_follow_the_spec_step_by_step(T, persistent):
    rows, ts = window_rows(T)
    cfg, w, eng, enc, states = _setup(T, rows)
    try:
        eng.set_option('persistent', persistent)
        S = 2 * T + 2
        _, _, _, align = eng.decode_greedy(mode=0, steps=S, want_align=True)
        lo, wk = eng.decode_greedy(mode=0, steps=S, want_align='sparse')[3]
        B, K = rows.shape[0], 2 * WIN + 1
        for j in range(B):
            for s in range(S):
                want = spec_window(ts[j], T) if s == 0 else spec_window_of_row(align[j, s - 1])
                assert _support_ok(align[j, s], want), (j, s, ts[j])
                if not want.any():
                    assert lo[j, s] == -1, (j, s)
                    continue
                first = int(np.argmax(want))
                assert lo[j, s] == first, (j, s)
                pat = np.zeros(K, bool)
                n = min(K, T - first)
                pat[:n] = want[first:first + n]
                assert np.array_equal(wk[j, s] != 0, pat), (j, s)
                assert np.array_equal(wk[j, s][:n][pat[:n]], align[j, s, first:first + n][pat[:n]]), (j, s)
    finally:
        eng.close()
