"""Cases, references and bounds of sampling under a cut (top_k, top_p) (csrc/sample_row.h: sample_row_cut_bound; csrc/sample_kernels.hip:
sample_cut_kernel; casv_decode_sample_cut, casv_debug_sample_cut_rows, casv_train_step_sampled_cut, casv_debug_sched_cut_rows; DESIGN.md
section 4.8, items 11 to 13) -- helpers, no test.  Held on the CPU by tests/test_sample_cut_cases.py, used on the device by
tests/test_gpu_sample_cut.py.  Everything stands on tests/sample_cases.py, which is imported and not changed.

  rank_masses       the definition's (a) and (b) restated in numpy: the rank order, the chunked rank-order prefix sums, the nucleus
  draw_rows         ... and (c): sample_cases.draw_rows at top_k = the row's kept places n (that IS the definition: the draw of a row
                    whose nucleus has n members is the draw at top_k = n)
  left_out          the ambiguity rule: sample_cases.left_out's, or some float64 rank-order prefix mass P_j / Z_s (j < n_a - 1) within
                    delta of top_p; delta = max(C_MAX * max|CDF32 - CDF64|, floor) -- the index-order CDFs for the draw, the
                    rank-order masses for the border
  under_cut         sample_cases' model comparison (reference_run, compare_draws, check_model, left_out_mask) with these two in
                    place of its own: its `top_k` argument then carries the cut

The floors.  Model runs: OLD_RT, as sample_cases.  Kernel-alone rows: KERNEL_FLOOR = 2^-20 -- the logits are given exactly, so only
expf's rounding separates the device from the restatement.  Measured with the float32 restatement against the float64 one on the CPU
(tests/test_sample_cut_cases.py asserts it on every kernel case): outside that margin the two never draw differently, and the left-out
share stays below LEFT_OUT_CAP on every case of KERNEL_CASES (at V = 4096 the rows are peaky -- scale 8 -- or cut to top_k <= 100 first:
a nucleus of 1 700 members of a flat row ends in a tail whose steps are smaller than any margin).
"""
import contextlib
from unittest import mock

import numpy as np

from tests import sample_cases as sa
from tests.decode_noise_cases import C_MAX, OLD_RT

LEFT_OUT_CAP = sa.LEFT_OUT_CAP
KERNEL_FLOOR = 2.0 ** -20
MAX_K = 4095
_plain_draw_rows = sa.draw_rows          # (under_cut puts this module's in its place)
SMALLEST_P = float(np.nextafter(np.float32(0), np.float32(1)))        # the smallest positive float32: the bits of top_k = 1


def rank_masses(x, tau, cut, dt=np.float64):
    """(a) and (b) on rows x (R,V): returns (n (R) kept places, order (R,V-1) the candidates' indices by rank, mass (R,V-1) the
    prefix masses P_j / Z_s of the places j < n_a and inf beyond, n_a).  Weights, sums and the product top_p * Z_s are formed in dt."""
    x = np.asarray(x)
    R, V = x.shape
    top_k, top_p = int(cut[0]), np.float32(cut[1])
    nc = V - 1
    order = np.argsort(-x[:, 1:], axis=1, kind='stable') + 1           # x descending, the lower index among equals, -0 == +0
    n_a = top_k if 0 < top_k < nc else nc
    n = np.full(R, n_a, np.int64)
    mass = np.full((R, nc), np.inf)
    if not top_p < 1 or nc < 1:
        return n, order, mass, n_a
    xd = x.astype(dt)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        mc = xd[:, 1:].max(axis=1)
        valid = ~np.isnan(xd).any(axis=1) & np.isfinite(mc)
        w = np.exp((np.take_along_axis(xd, order, axis=1) - mc[:, None]) / dt(np.float32(tau))).astype(dt)
    w[~valid] = 0
    chunk = (V + 63) // 64                                               # lane l owns the places [l * chunk, (l + 1) * chunk)
    padded = np.zeros((R, 64 * chunk), dt)
    padded[:, :n_a] = w[:, :n_a]
    run = np.cumsum(padded.reshape(R, 64, chunk), axis=2, dtype=dt)      # a lane's weights in ascending place order
    c = run[:, :, -1]
    off = np.concatenate([np.zeros((R, 1), dt), np.cumsum(c, axis=1, dtype=dt)[:, :-1]], axis=1)      # one sequential pass over the lanes
    P = (off[:, :, None] + run).reshape(R, -1)[:, :n_a]
    Zs = P[:, n_a - 1]
    target = dt(top_p) * Zs                                             # (formed once, in dt)
    reach = P >= target[:, None]
    jstar = np.where(reach.any(axis=1), reach.argmax(axis=1), n_a - 1)
    n = np.where(valid, jstar + 1, n_a)
    with np.errstate(invalid='ignore', divide='ignore'):
        mass[:, :n_a] = np.where(valid[:, None], P / np.where(valid, Zs, 1)[:, None], np.inf)
    return n, order, mass, n_a


def draw_rows(x, u, tau=1.0, cut=(0, 1.0), dt=np.float64):
    """The draw of every row of x (R,V) under the cut at the uniforms u (R): sample_cases.draw_rows' dict, and n (R) the kept places,
    mass (R,V-1) the rank-order prefix masses, n_a, cut."""
    x = np.asarray(x)
    R, V = x.shape
    u = np.broadcast_to(np.asarray(u), (R,))
    n, order, mass, n_a = rank_masses(x, tau, cut, dt)
    out = None
    for k in np.unique(n):
        rows = np.nonzero(n == k)[0]
        d = _plain_draw_rows(x[rows], u[rows], tau, int(k) if 0 < k < V - 1 else 0, dt)
        if out is None:
            out = {key: np.empty((R,) + np.shape(val)[1:], np.asarray(val).dtype) for key, val in d.items()}
        for key, val in d.items():
            out[key][rows] = val
    out.update(n=n, mass=mass, n_a=n_a, cut=(int(cut[0]), float(np.float32(cut[1]))))
    return out


def left_out(u, d64, d32, floor=OLD_RT):
    """(left out (R) bool, distance (R) of u from the nearest interior boundary of the float64 CDF): sample_cases.left_out's rule at
    this floor, or a rank-order prefix mass of a place j < n_a - 1 within delta of top_p."""
    u = np.asarray(u, np.float64)
    same = (d64['cand'] == d32['cand']).all(axis=1)
    c = np.asarray(d64['cdf'], np.float64)
    delta = np.maximum(C_MAX * np.abs(np.asarray(d32['cdf'], np.float64) - c).max(axis=1), floor)
    interior = d64['cand'] & (c > 0) & (c < 1)
    dist = np.where(interior, np.abs(u[:, None] - c), np.inf).min(axis=1)
    out = ~same | (dist <= delta)
    top_p, n_a = d64['cut'][1], d64['n_a']
    if top_p < 1 and n_a > 1:
        m64, m32 = d64['mass'][:, :n_a - 1], d32['mass'][:, :n_a - 1]
        with np.errstate(invalid='ignore'):
            dev = np.where(np.isfinite(m64) & np.isfinite(m32), np.abs(m32 - m64), 0).max(axis=1)
            delta_p = np.maximum(C_MAX * dev, floor)
            out |= (np.abs(m64 - top_p) <= delta_p[:, None]).any(axis=1)
    return out, dist


@contextlib.contextmanager
def under_cut(floor=OLD_RT):
    """sample_cases' comparisons with this module's draw_rows and left_out: inside, their `top_k` argument is the cut."""
    with mock.patch.object(sa, 'draw_rows', draw_rows), \
            mock.patch.object(sa, 'left_out', lambda u, d64, d32: left_out(u, d64, d32, floor)):
        yield


def check_model(case, got, tau, cut, seed, **kw):
    with under_cut():
        return sa.check_model(case, got, tau, cut, seed, **kw)


def reference_run(case, tau, cut, seed, **kw):
    with under_cut():
        return sa.reference_run(case, tau, cut, seed, **kw)


def compare_draws(ref, seq, tau, cut, reported):
    with under_cut():
        return sa.compare_draws(ref, seq, tau, cut, reported)


def cap_rows(R):
    """How many of a kernel case's own R rows may be left out: the cap, and one row of a batch too small for a share to mean much."""
    return max(int(LEFT_OUT_CAP * R), 1 if R < 20 else 0)


def sched_next_mix(case, current, gold, ratio, tau, cut, seed=None, step_id=None):
    """tests/sched_cases.next_mix for the sampled pick under a cut: one pass of the definition on the float64 oracle from the decoder
    input `current` (B,U) -> (mix (B,U), left out (B,U) bool), the float32 oracle deciding the margin (floor OLD_RT)."""
    from tests import sched_cases as sc
    seed = sc.SEED if seed is None else seed
    step_id = sc.STEP_ID if step_id is None else step_id
    gold = np.asarray(gold)
    B, U = gold.shape
    prev = lambda a: np.concatenate([a[:, :1], a[:, :-1]], axis=1).reshape(B * U, -1)        # row of position (b, u - 1); u = 0 unused
    x64, x32 = prev(sc.logp(case, current, np.float64)), prev(sc.logp(case, current, np.float32)).astype(np.float32)
    bb, uu = np.repeat(np.arange(B), U), np.tile(np.arange(U), B)
    c, u2 = sc.coins(seed, step_id, bb, uu)
    d64, d32 = draw_rows(x64, u2, tau, cut), draw_rows(x32, u2, tau, cut, np.float32)
    replaced = (uu >= 1) & (gold.reshape(-1) >= 0) & (c < np.float32(ratio)) & d64['valid']
    out = left_out(u2, d64, d32)[0] & replaced
    return np.where(replaced, d64['idx'], gold.reshape(-1)).astype(np.int32).reshape(B, U), out.reshape(B, U)


# ------------------------------------------------------------------------------------------------------------------ the kernel alone
# (V, R, (top_k, top_p), tau, logit scale): every V, R and cut of the issue at least once ("V-2" and 4095 by their values); R = 1000 and
# 37: more than one workgroup; 5 / 3 / 1 / 4: a partial last workgroup for each rows-per-workgroup value (4 up to V = 2048, 3 at 4096;
# the option "sample_cut_rows" brings 2 and 1).  At V = 4096 the rows are peaky (scale 8) or top_k <= 100 stands in front of the nucleus.
KERNEL_CASES = [(2, 5, (0, 0.5), 1.0, 2.0), (2, 1, (4095, 1.0), 1.0, 2.0),
                (12, 1, (0, 0.5), 1.0, 2.0), (12, 5, (5, 0.9), 0.5, 2.0), (12, 3, (10, 1.0), 1.0, 2.0), (12, 4, (65, 1.0), 2.0, 2.0),
                (40, 1000, (0, 0.9), 1.0, 3.0), (40, 5, (38, 1.0), 1.0, 3.0), (40, 4, (5, 0.9), 0.5, 3.0), (40, 3, (4095, 1.0), 2.0, 3.0),
                (64, 5, (0, 0.5), 1.0, 3.0), (64, 4, (62, 1.0), 2.0, 3.0), (64, 37, (0, 0.9), 0.5, 3.0),
                (65, 5, (0, 0.9), 0.5, 3.0), (65, 4, (65, 1.0), 1.0, 3.0), (65, 1, (63, 1.0), 1.0, 3.0), (65, 3, (5, 0.9), 2.0, 3.0),
                (96, 5, (65, 1.0), 1.0, 4.0), (96, 37, (0, 0.5), 2.0, 4.0), (96, 4, (94, 1.0), 0.5, 4.0),
                (640, 5, (0, 0.9), 1.0, 4.0), (640, 3, (65, 1.0), 0.5, 4.0), (640, 4, (638, 1.0), 1.0, 4.0), (640, 37, (5, 0.9), 2.0, 4.0),
                (4096, 5, (0, 0.9), 1.0, 8.0), (4096, 3, (65, 1.0), 2.0, 3.0), (4096, 1, (4094, 1.0), 1.0, 3.0), (4096, 4, (4095, 1.0), 1.0, 3.0),
                (4096, 37, (100, 0.9), 2.0, 3.0), (4096, 4, (0, 0.5), 0.5, 8.0)]
KERNEL_IDS = ['V%d_R%d_k%d_p%g_t%g' % (c[0], c[1], c[2][0], c[2][1], c[3]) for c in KERNEL_CASES]


def kernel_case(c):
    """Rows x (R,V) of a kernel case, their stream ids (beyond 2^32 among them), sample numbers, step and seed."""
    V, R, cut, tau, scale = c
    rng = np.random.default_rng(1000 * V + R + cut[0])
    x = (rng.standard_normal((R, V)) * scale).astype(np.float32)
    streams = rng.integers(0, 2 ** 40, R).astype(np.int64)
    samples = rng.integers(0, 64, R).astype(np.int32)
    return x, streams, samples, int(rng.integers(0, 200)), int(rng.integers(0, 2 ** 63))


def constructed_rows():
    """[(name, x (V,), cut, tau, facts)]: what the definition says of the row whatever u is -- `valid`, `only` (the indices that can be
    drawn), `never`.  Exact, with no margin."""
    rng = np.random.default_rng(29)
    rows = []

    def base(V, lo=-3.0, hi=-1.0):
        return rng.uniform(lo, hi, V).astype(np.float32)
    eq = np.full(40, 1.5, np.float32)                   # 39 weights of exactly 1: 0.25 * 39 = 9.75, first reached by place 9
    rows.append(('equal_p025', eq, (0, 0.25), 1.0, dict(valid=True, only=tuple(range(1, 11)))))
    rows.append(('equal_k5_p05', eq, (5, 0.5), 1.0, dict(valid=True, only=(1, 2, 3))))           # 0.5 * 5 = 2.5: places 0 .. 2
    x = base(40); x[17] = 6.0                            # the maximum alone exceeds p: e^-7 * 38 others < 0.1 of the total
    rows.append(('maximum_alone', x, (0, 0.9), 1.0, dict(valid=True, only=(17,))))
    # a tie group straddling the border is entered in index order: weights 1 (index 20) and e^-2 = 0.1353 each for {3, 9, 31, 38}, the
    # other 34 at most e^-10 each, so Z lies in [1.5413, 1.5429] and 0.85 Z in [1.3101, 1.3115]: above P_2 = 1.2707, below P_3 = 1.4060
    x = base(40, -9.0, -6.0); x[20] = 4.0; x[[38, 3, 31, 9]] = 2.0
    rows.append(('tie_at_the_border', x, (0, 0.85), 1.0, dict(valid=True, only=(20, 3, 9, 31))))
    x = base(40); x[[4, 30]] = 0.0; x[[2, 9, 35]] = -0.0; x[x < 0] -= 9      # five equal zeros of either sign: 0.5 * ~5 -> places 0 .. 2
    rows.append(('mixed_zeros', x, (0, 0.5), 1.0, dict(valid=True, only=(2, 4, 9))))
    x = np.full(40, -np.inf, np.float32); x[[7, 12, 33, 39]] = (-1.5, 0.25, -1.5, -4.0)
    rows.append(('minus_inf_members', x, (0, float(np.nextafter(np.float32(1), np.float32(0)))), 1.0, dict(valid=True, only=(7, 12, 33, 39))))
    rows.append(('minus_inf_members_k8', x, (8, float(np.nextafter(np.float32(1), np.float32(0)))), 1.0, dict(valid=True, only=(7, 12, 33, 39))))
    x = base(40); x[0] = 50.0; x[23] = 5.0
    rows.append(('index_0_largest', x, (0, 0.5), 1.0, dict(valid=True, only=(23,))))
    for at in (0, 17, 39):
        x = base(40); x[at] = np.nan
        rows.append(('nan_at_%d' % at, x, (0, 0.9), 1.0, dict(valid=False)))
    x = base(40); x[11] = np.inf
    rows.append(('plus_inf', x, (0, 0.9), 1.0, dict(valid=False)))
    rows.append(('all_minus_inf', np.full(40, -np.inf, np.float32), (0, 0.9), 1.0, dict(valid=False)))
    x = np.full(40, -np.inf, np.float32); x[0] = 1.0
    rows.append(('only_index_0_finite', x, (5, 0.9), 1.0, dict(valid=False)))
    rows.append(('v2', np.array([3.0, -1.0], np.float32), (0, 0.5), 1.0, dict(valid=True, only=(1,))))
    rows.append(('v2_k', np.array([3.0, -1.0], np.float32), (4095, 1.0), 1.0, dict(valid=True, only=(1,))))
    x = base(640); x[[69, 581, 133, 5, 639]] = 2.0; x[0] = 9.0
    first = tuple(int(v) for v in (np.argsort(-x[1:], kind='stable') + 1))
    for k in (65, 100, 638):
        rows.append(('v640_k%d' % k, x, (k, 1.0), 1.0, dict(valid=True, only=first[:k], never=first[k:] + (0,))))
    rows.append(('k_at_least_all', base(40), (39, 1.0), 1.0, dict(valid=True, never=(0,))))
    rows.append(('k_beyond_all', base(40), (4095, 1.0), 1.0, dict(valid=True, never=(0,))))
    x = base(65)
    rows.append(('cold', x, (0, 0.9), 1e-3, dict(valid=True, only=(1 + int(x[1:].argmax()),))))
    return rows


# ------------------------------------------------------------------------------------------------------------------ the model
# (case of sample_cases.MODEL_CASES, tau, cut): the issue's eleven, each within LEFT_OUT_CAP on the reference alone
# (tests/test_sample_cut_cases.py asserts it)
_BY_NAME = {c[0]: c for c in sa.MODEL_CASES}
MODEL_DRAWS = [(_BY_NAME['d1_w32_v12'], 1.0, (0, 0.9)),
               (_BY_NAME['d2_w64_v40_unequal'], 1.0, (0, 0.8)),
               (_BY_NAME['d2_w64_v40_unequal'], 1.0, (20, 0.8)),
               (_BY_NAME['d2_w64_v40_unequal'], 0.5, (0, 0.5)),
               (_BY_NAME['d3_w64_v40_rows15'], 0.5, (0, 0.5)),
               (_BY_NAME['d2_w128_v96'], 0.5, (0, 0.5)),
               (_BY_NAME['d2_w128_v96'], 0.5, (70, 0.5)),
               (_BY_NAME['residual_d3_w64'], 0.5, (0, 0.5)),
               (_BY_NAME['bridge_d2_w64'], 0.5, (0, 0.5)),
               (_BY_NAME['deep_d2_w64'], 0.5, (0, 0.5)),
               (_BY_NAME['confusion_d2_w64'], 0.5, (0, 0.5))]
MODEL_DRAW_IDS = ['%s_t%g_k%d_p%g' % (c[0], tau, cut[0], cut[1]) for c, tau, cut in MODEL_DRAWS]
