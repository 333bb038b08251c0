"""Cases, references and rules of scheduled sampling inside the train step (csrc/sched_kernels.hip: sched_mix_kernel; csrc/train.hip:
casv_train_step_sampled, casv_debug_sched_rows) -- helpers, no test.  Held on the CPU by
tests/test_sched_cases.py, used on the device by tests/test_gpu_sched.py.

  coins                     the coin and the draw's uniform of position (b, u): words 0 and 1 of tests/sample_cases.py's Philox
  mix_rows                  the definition restated on rows of logits (or log-probabilities): greedy exactly, sampled by draw_rows
  sampled_left_out          left_out's rule for the sampled pick of rows
  constructed_rows          the kernel-alone rows built by hand, with what the definition says of each
  STEP_CASES, build         the step's cases (the issue's table); logp() = the oracle's teacher-forced log-probabilities of a decoder
                            input given as indices; next_mix() = one pass of the definition on them, with the positions left out
  sequential                the sequential procedure (Bengio et al. 2015) on the oracle, step by step
  parallel                  the parallel procedure (Duckworth et al. 2019) on the oracle, pass by pass

The rule for a greedy position: float32 and float64 logits of a row differ by at most dev = max_v |x32_v - x64_v| (measured per row,
the float32 oracle against the float64 one on the same decoder input); the device is allowed C_MAX such units, as
tests/decode_noise_cases.py allows its probabilities, floored at its old relative tolerance OLD_RT.  Two entries can change places
only if each moves by half their gap, so a position is left out where the float64 top-two gap among the candidates is at most
2 x max(C_MAX x dev, OLD_RT).  The sampled rule is tests/sample_cases.left_out unchanged."""
import functools

import numpy as np

from oracle import ModelConfig, make_weights, make_lines, vectorize_lines
from oracle.decode import OracleModel
from oracle.train import forward_backward
from tests.decode_noise_cases import C_MAX, OLD_RT
from tests.sample_cases import LEFT_OUT_CAP, MASK, draw_rows, left_out, philox4x32_10          # noqa: F401 (LEFT_OUT_CAP: for the tests)


# ------------------------------------------------------------------------------------------------------------------ the generator
def coins(seed, step_id, b, u):
    """(coin uniform, draw uniform) float32 of positions (b, u), broadcast: (o0 >> 8) 2^-24 and (o1 >> 8) 2^-24 of Philox4x32-10 on
    the counter (step_id low, step_id high, b, u) under the key (seed low, seed high)."""
    seed, step_id = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step_id) & 0xFFFFFFFFFFFFFFFF
    b, u = np.broadcast_arrays(np.asarray(b, np.uint64), np.asarray(u, np.uint64))
    o = philox4x32_10((np.full(b.shape, step_id & MASK, np.uint64), np.full(b.shape, step_id >> 32, np.uint64), b, u), (seed & MASK, seed >> 32))
    f = lambda w: ((w >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    return f(o[0]), f(o[1])


# ------------------------------------------------------------------------------------------------------------------ the definition
def greedy_rows(x):
    """(pick (R), valid (R), float64 top-two gap among the candidates (R); inf with one candidate) of rows x (R,V): the largest x_v over
    v = 1 .. V-1, the lowest index among equals (-0 == +0: numpy compares them equal); invalid = a NaN in the row or a candidates'
    maximum that is not finite."""
    x = np.asarray(x)
    R, V = x.shape
    xd = x.astype(np.float64)
    if V < 2:
        return np.ones(R, np.int32), np.zeros(R, bool), np.full(R, np.inf)
    with np.errstate(invalid='ignore'):
        c = xd[:, 1:]
        pick = np.argmax(np.where(np.isnan(c), -np.inf, c), axis=1) + 1
        mc = c.max(axis=1)
        valid = ~np.isnan(xd).any(axis=1) & np.isfinite(mc)
        srt = np.sort(np.where(np.isnan(c), -np.inf, c), axis=1)
        gap = srt[:, -1] - srt[:, -2] if V > 2 else np.full(R, np.inf)
    return pick.astype(np.int32), valid, np.where(valid, gap, np.inf)


def mix_rows(x, gold, b, u, seed, step_id, ratio, pick='greedy', tau=1.0, dt=np.float64):
    """The definition on rows: x (R,V) logits (or log-probabilities) of the position BEFORE (b[r], u[r]), gold (R).  Returns
    dict(mix (R) int32, coin (R) bool, eligible, valid, replaced; greedy: gap; sample: draw = draw_rows' dict, u2)."""
    gold, b, u = (np.asarray(a) for a in (gold, b, u))
    c, u2 = coins(seed, step_id, b, u)
    coin = c < np.float32(ratio)
    eligible = (u >= 1) & (gold >= 0)
    out = dict(coin=coin, eligible=eligible, u2=u2)
    if pick == 'greedy':
        idx, valid, gap = greedy_rows(x)
        out['gap'] = gap
    else:
        d = draw_rows(np.asarray(x), u2, tau, 0, dt)
        idx, valid = d['idx'], d['valid']
        out['draw'] = d
    out['valid'] = valid
    out['replaced'] = eligible & coin & valid
    out['mix'] = np.where(out['replaced'], idx, gold).astype(np.int32)
    return out


def sampled_left_out(x64, x32, u2, tau):
    """tests/sample_cases.left_out on the rows' float64 and float32 logits (or log-probabilities): (R) bool."""
    return left_out(u2, draw_rows(x64, u2, tau, 0, np.float64), draw_rows(x32, u2, tau, 0, np.float32))[0]


def constructed_rows(V):
    """[(name, x (V,), gold, u, fact)] at vocabulary size V >= 2; fact: 'gold' = the row keeps its gold value whatever the coin,
    an int = the greedy pick where the coin is true."""
    rng = np.random.default_rng(1000 + V)
    base = lambda: rng.uniform(-3.0, -1.0, V).astype(np.float32)
    g = 1 + (V - 1) // 2            # a gold index among the candidates
    rows = []
    x = base(); x[V - 1] = 2.0
    rows.append(('max_last', x, g, 1, V - 1))
    x = base(); x[0] = 9.0; x[1] = 1.0
    rows.append(('max_at_index_0', x, g, 2, 1))
    if V >= 4:
        x = base(); x[[V - 1, 2, V - 2]] = 2.0
        rows.append(('tie_lower_index', x, g, 3, 2))
        x = np.full(V, -5.0, np.float32); x[V - 1] = 0.0; x[2] = -0.0
        rows.append(('zeros_equal', x, g, 1, 2))
        x = np.full(V, -np.inf, np.float32); x[V - 2] = -7.0
        rows.append(('one_finite', x, g, 4, V - 2))
    rows.append(('all_equal', np.full(V, 1.5, np.float32), g, 1, 1))
    for at in sorted({0, V // 2, V - 1}):
        x = base(); x[at] = np.nan
        rows.append(('nan_at_%d' % at, x, g, 1, 'gold'))
    rows.append(('all_minus_inf', np.full(V, -np.inf, np.float32), g, 2, 'gold'))
    x = np.full(V, -np.inf, np.float32); x[0] = 1.0
    rows.append(('only_index_0_finite', x, g, 2, 'gold'))
    x = base(); x[1] = np.inf
    rows.append(('plus_inf', x, g, 2, 'gold'))
    rows.append(('gold_minus_1', base(), -1, 3, 'gold'))
    rows.append(('u_0', base(), g, 0, 'gold'))
    rows.append(('u_0_gold_minus_1', base(), -1, 0, 'gold'))
    return rows


KERNEL_V = (2, 12, 33, 256, 4096)
KERNEL_GRID = ((0, 0), (1, 1 << 32), ((1 << 63) + 12345, (1 << 40) + 7), (99, 3))         # (seed, step_id)
KERNEL_DRAWS = (('greedy', 1.0), ('sample', 1.0), ('sample', 0.3))                         # (pick, temperature)


def random_rows(V, R=37):
    """R random rows at vocabulary size V (more than one workgroup of four waves, a partial last one), positions with u = 0 and gold
    -1 among them, batch rows beyond 2^16.  The logits' scale is 3, and 6 at V = 4096: there a row at scale 3 has so many CDF
    boundaries within OLD_RT of each other that left_out's rule takes 6 of 92 draws, past the cap (tests/test_sched_cases.py)."""
    rng = np.random.default_rng(7 * V + R)
    x = (rng.standard_normal((R, V)) * (3.0 if V <= 256 else 6.0)).astype(np.float32)
    gold = rng.integers(1, V, R).astype(np.int32)
    gold[rng.random(R) < 0.15] = -1
    b = rng.integers(0, 1 << 20, R).astype(np.int32)
    u = rng.integers(0, 200, R).astype(np.int32)
    u[rng.random(R) < 0.15] = 0
    return x, gold, b, u


# ------------------------------------------------------------------------------------------------------------------ the step
# (name, depth, width, V, source characters per line, target characters kept, flags, masks): T = longest source + 1, U = kept + 2
STEP_CASES = [('d%d_w32_v12' % d, d, 32, 12, (1, 4, 6), 4, (), False) for d in (1, 2, 3)]
STEP_CASES += [('d3_w32_v12_residual_bridge', 3, 32, 12, (1, 4, 6), 4, ('residual_connections', 'bridge_dense'), False),
               ('d2_w64_v40_masks', 2, 64, 40, (7, 3, 8, 8, 5), 6, (), True)]
STEP_IDS = [c[0] for c in STEP_CASES]
SEED, STEP_ID = 0x5EED5EED5EED, (1 << 32) + 5
SEQ_CASE = STEP_CASES[1]            # sequential equivalence: U = 6, passes = 5, greedy, ratio 0.5


@functools.lru_cache(maxsize=None)
def build(case, seed=4):
    """cfg, float32 weights, oracle inputs (enc_in, dec_in, dec_out, wts, masks), device batch (idx, val, dec_in, dec_out, wts, masks)
    of a case, as tests/grad_noise_cases.build builds them, on lines of the case's lengths."""
    name, d, W, V, lens, keep, flags, with_masks = case
    B = len(lens)
    cfg = ModelConfig(depth=d, width=W, voc_size=V, **{f: True for f in flags})
    w = make_weights(cfg, emb_scale=4.0)
    rng = np.random.default_rng(seed)
    for k in w:
        if k.endswith('_b') or k in ('att_bUW', 'att_bv'):
            w[k] = (w[k] + rng.normal(size=w[k].shape) * 0.2).astype(np.float32)
    om = OracleModel(cfg, w)
    full, _ = make_lines(B, max(lens), 1, voc_size=V)
    src = [l[:n] + '\n' for l, n in zip(full, lens)]
    tgt = [l[:min(n, keep)] + '\n' for l, n in zip(full, lens)]
    enc_in, dec_in, dec_out, wts = vectorize_lines(om, src, tgt)
    idx = lambda a: np.where(a.any(axis=2), a.argmax(axis=2), -1).astype(np.int32)
    masks = None
    if with_masks:
        C = cfg.ctx_width
        keep_ = lambda shape: ((rng.random(shape) > 0.2) / 0.8).astype(np.float32)
        masks = {'enc': [keep_(2 * W if n == 0 else W) for n in range(d)], 'dec': [keep_(W) for _ in range(d - 1)], 'cell': keep_((B, W + C))}
    assert enc_in.shape[1] == max(lens) + 1 and dec_in.shape[1] == min(max(lens), keep) + 2
    return cfg, w, (enc_in, dec_in, dec_out, wts, masks), (idx(enc_in), None, idx(dec_in), idx(dec_out), wts, masks)


def onehot(index, V, dtype=np.float32):
    """(B,U) indices, -1 = zero row -> (B,U,V) one-hot rows."""
    index = np.asarray(index)
    out = np.zeros(index.shape + (V,), dtype)
    bb, uu = np.nonzero(index >= 0)
    out[bb, uu, index[bb, uu]] = 1
    return out


def oracle_inputs(case, dec_in_index):
    """The case's oracle inputs with the decoder input replaced by the one-hot rows of dec_in_index (B,U)."""
    cfg, w, (enc_in, _, dec_out, wts, masks), _ = build(case)
    return enc_in, onehot(dec_in_index, cfg.voc_size), dec_out, wts, masks


def logp(case, dec_in_index, dtype):
    """(B,U,V) log-probabilities of the teacher-forced oracle forward in `dtype` (window decided in float32) on the decoder input
    dec_in_index (B,U) and the case's masks: the logits up to a constant per row, which no pick depends on."""
    cfg, w, _, _ = build(case)
    enc_in, dec_in, dec_out, wts, masks = oracle_inputs(case, dec_in_index)
    cast = lambda a: np.asarray(a, dtype)
    m = None if masks is None else {'enc': [cast(x) for x in masks['enc']], 'dec': [cast(x) for x in masks['dec']], 'cell': cast(masks['cell'])}
    _, _, aux = forward_backward(cfg, {k: cast(v) for k, v in w.items()}, cast(enc_in), cast(dec_in), cast(dec_out), cast(wts), m,
                                 want_grads=False, window_dtype=np.float32)
    with np.errstate(divide='ignore'):
        return np.log(np.asarray(aux['probs'], np.float64))


def next_mix(case, current, gold, ratio, pick='greedy', tau=1.0, seed=SEED, step_id=STEP_ID, dtype=np.float64):
    """One pass of the definition on the oracle: (mix (B,U), left out (B,U) bool) from the decoder input `current` (B,U).  The
    rules of the module docstring decide what is left out (only positions whose coin is true and that are eligible can be)."""
    gold = np.asarray(gold)
    B, U = gold.shape
    x64 = logp(case, current, np.float64)
    x = x64 if dtype == np.float64 else logp(case, current, np.float32)
    x32 = logp(case, current, np.float32)
    prev = lambda a: np.concatenate([a[:, :1], a[:, :-1]], axis=1).reshape(B * U, -1)        # row of position (b, u - 1); u = 0 unused
    bb, uu = np.repeat(np.arange(B), U), np.tile(np.arange(U), B)
    r = mix_rows(prev(x), gold.reshape(-1), bb, uu, seed, step_id, ratio, pick, tau)
    if pick == 'greedy':
        r64 = r if dtype == np.float64 else mix_rows(prev(x64), gold.reshape(-1), bb, uu, seed, step_id, ratio, pick, tau)
        dev = np.abs(prev(x32) - prev(x64))
        dev = np.where(np.isfinite(dev), dev, 0.0).max(axis=1)
        out = r64['gap'] <= 2 * np.maximum(C_MAX * dev, OLD_RT)
    else:
        out = sampled_left_out(prev(x64), prev(x32).astype(np.float32), r['u2'], tau)
    return r['mix'].reshape(B, U), (out & r['eligible'] & r['coin']).reshape(B, U)


def parallel(case, gold, ratio, passes, **kw):
    """The parallel procedure on the oracle: ([mix after pass 1 .. passes], [left out of each pass])."""
    cur, mixes, outs = np.asarray(gold), [], []
    for _ in range(passes):
        cur, lo = next_mix(case, cur, gold, ratio, **kw)
        mixes.append(cur); outs.append(lo)
    return mixes, outs


def sequential(case, gold, ratio, **kw):
    """The sequential procedure on the oracle: position u of the input is decided from the logits of position u - 1 of the forward
    pass on the input decided so far (causal: those logits read positions <= u - 1 only).  (input (B,U), left out (B,U))."""
    gold = np.asarray(gold)
    U = gold.shape[1]
    cur, out = gold.copy(), np.zeros(gold.shape, bool)
    for u in range(1, U):
        mix, lo = next_mix(case, cur, gold, ratio, **kw)
        cur[:, u], out[:, u] = mix[:, u], lo[:, u]
    return cur, out
