"""The decode path (encoder, decoder step, LM step) against a float64 run of the oracle, in units of the fp32 oracle's own rounding
noise (tests/test_gpu_decode_noise.py, tests/test_decode_noise_bounds.py, profiles/decode_noise.py) -- the decode-side counterpart of
tests/grad_noise_cases.py.

o64 = the oracle on float64 weights and inputs, with the attention window decided by the spec's fp32 rule (window_dtype=float32:
t' rounded once to float32, membership tested in float32); o32 = the same in float32.  Every decoder step starts from the same
float32 inputs for the device, o32 and o64: the fp32 oracle's previous outputs (teacher forcing).
- Encoder outputs, final states, and after each step every h_n / c_n and the alignment row: absolute error against o64 in units of
  the fp32 oracle's (rms, max) error, each unit floored at 2^-24 max|o64|.
- Decoder and LM probabilities: relative error (p - p64) / p64 where p64 >= 1e-30, in units of the fp32 oracle's relative error,
  floored at 2^-24.
- NaN entries (empty windows) must be NaN on the device exactly where o32 has them; they are left out of the ratios."""
import contextlib

import numpy as np

from oracle import ModelConfig, make_weights, make_lines
import oracle.model as om_model
from oracle.model import encode, decoder_step
from oracle.decode import OracleModel
from tests.lm_oracle import lm_step

# measured on an MI355X (profiles/r09_decode_noise.txt): largest rms ratio 1.495 (encoder output, 100-character lines at W = 512),
# largest max ratio 2.674 (c1 of the depth-1 step, arithmetic 0); the constants are 2x those, rounded up (two runs gave the same
# bits); they may not exceed the train step's caps (16 / 64)
C_RMS, C_MAX = 3.0, 6.0
OLD_RT, OLD_AT = 2e-4, 2e-6        # the per-step tolerance of tests/test_gpu_parity.py (recorded for the mutations, not asserted)
CHUNK = 2048                       # rows per oracle call (the dense attention holds R x T x W values)

# (name, depth, width, voc, lines, length, flags, alternatives, arithmetic, persistent)
ENC_CASES = [
    ('persist_d2_w256_b64', 2, 256, 40, 64, 40, {}, 1, 0, -1),
    ('stepwise_d2_w256_b1024', 2, 256, 40, 1024, 20, {}, 1, 0, -1),
    ('stepwise_p0_d3_w128_b32', 3, 128, 40, 32, 24, {}, 1, 0, 0),
    ('split_d2_w512_b1024', 2, 512, 40, 1024, 16, {}, 1, 2, -1),
    ('split_small_d2_w128_b64', 2, 128, 40, 64, 20, {}, 1, 2, -1),
    ('d1_w256_b48', 1, 256, 40, 48, 24, {}, 1, 0, -1),
    ('w100_d2_b40', 2, 100, 40, 40, 24, {}, 1, 0, -1),
    ('residual_d4_w64', 4, 64, 96, 24, 20, dict(residual_connections=True), 1, 0, -1),
    ('bridge_d3_w64', 3, 64, 40, 24, 20, dict(bridge_dense=True), 1, 0, -1),
    ('deep_d3_w96', 3, 96, 40, 24, 20, dict(deep_bidirectional_encoder=True), 1, 0, -1),
    ('confusion_d3_w64', 3, 64, 40, 24, 20, {}, 2, 0, -1),
    ('long_d2_w512_b8_l100', 2, 512, 96, 8, 100, {}, 1, 0, -1),
]

# (name, depth, width, voc, rows, positions, lines, steps); every case runs under arithmetic 0 and 2
STEP_CASES = [
    ('r37_d2_w256_v40', 2, 256, 40, 37, 20, 7, 3),
    ('r1000_d1_w512_v256', 1, 512, 256, 1000, 24, 125, 2),
    ('r8191_d4_w256_v40', 4, 256, 40, 8191, 16, 1024, 2),
    ('r8192_d2_w512_v640', 2, 512, 640, 8192, 16, 1024, 1),
    ('page_r10240_d2_w512_v256', 2, 512, 256, 10240, 16, 40, 1),     # 320 tiles of 256x256 under arithmetic 2: the partial-round cut
]


def _rms(x):
    return float(np.sqrt(np.mean(x ** 2))) if x.size else 0.0


def ratio(got, o32, o64, rel=False):
    """(rms ratio, max ratio) of got against o64 in units of o32's error (module docstring); NaN entries of o32 / o64 left out."""
    g, a, r = (np.asarray(x, np.float64) for x in (got, o32, o64))
    m = ~(np.isnan(a) | np.isnan(r))
    if rel:
        m &= np.abs(r) >= 1e-30
        e, n, floor = (g[m] - r[m]) / r[m], (a[m] - r[m]) / r[m], 2.0 ** -24
    else:
        e, n = g[m] - r[m], a[m] - r[m]
        floor = 2.0 ** -24 * max(float(np.abs(r[m]).max()) if m.any() else 0.0, 1e-30)
    if not m.any():
        return 0.0, 0.0
    return _rms(e) / max(_rms(n), floor), float(np.abs(e).max()) / max(float(np.abs(n).max()), floor)


def excess(r):
    """How far ratios {quantity: (rms, max)} go past the bound: max of ratio / constant (< 1: within)."""
    return max(max(a / C_RMS, b / C_MAX) for a, b in r.values())


def nan_mismatch(got, o32):
    """Quantities whose NaN entries differ between the device and the fp32 oracle."""
    return [k for k in o32 if not np.array_equal(np.isnan(np.asarray(got[k])), np.isnan(np.asarray(o32[k])))]


def ratios(got, o32, o64):
    return {k: ratio(got[k], o32[k], o64[k], rel=k in ('probs', 'lm')) for k in o64}


def old_catches(got, o64):
    """Whether the old per-step tolerance (rtol 2e-4, atol 2e-6 against the oracle) would flag `got`."""
    return any(not np.allclose(np.asarray(got[k], np.float64), o64[k], rtol=OLD_RT, atol=OLD_AT, equal_nan=True) for k in o64)


# ---------------------------------------------------------------------------------------------------------------------------
# encoder

def build_encoder(case, seed=3):
    """cfg, float32 weights, oracle input x (B,T,V) and device input (idx, val)."""
    name, d, W, V, B, L, flags, A, arith, persistent = case
    cfg = ModelConfig(depth=d, width=W, voc_size=V, **flags)
    w = make_weights(cfg, emb_scale=4.0)
    rng = np.random.default_rng(seed)
    for k in w:
        if k.endswith('_b') or k in ('att_bUW', 'att_bv'):
            w[k] = (w[k] + rng.normal(size=w[k].shape) * 0.2).astype(np.float32)
    _, sidx = make_lines(B, L, seed, voc_size=V)
    x = np.zeros(sidx.shape + (V,), np.float32)
    bb, tt = np.nonzero(sidx >= 0)
    if A == 1:
        x[bb, tt, sidx[bb, tt]] = 1.0
        return cfg, w, x, (sidx, None)
    alt = np.where(sidx >= 0, np.roll(sidx, 1, axis=1), -1)        # confusion network: two alternatives, 0.75 / 0.25
    alt = np.where(alt >= 0, alt, sidx)
    x[bb, tt, sidx[bb, tt]] += 0.75
    x[bb, tt, alt[bb, tt]] += 0.25
    val = np.stack([np.full(alt.shape, 0.75), np.full(alt.shape, 0.25)], axis=2).astype(np.float32)
    return cfg, w, x, (np.stack([sidx, alt], axis=2).astype(np.int32), val)


def oracle_encoder(cfg, w, x, dtype):
    out = encode(cfg, {k: np.asarray(v, dtype) for k, v in w.items()}, np.asarray(x, dtype))
    q = {'enc_out': out[0]}
    for n in range(cfg.depth):
        q['h%d' % (n + 1)], q['c%d' % (n + 1)] = out[1 + 2 * n], out[2 + 2 * n]
    return q


def device_encoder(case, w, inputs):
    from cor_asv_ann_amd.engine import HipEngine
    name, d, W, V, B, L, flags, A, arith, persistent = case
    eng = HipEngine(d, W, V, **flags)
    try:
        eng.set_weights(w)
        eng.set_option('arithmetic', arith)
        eng.set_option('persistent', persistent)
        eng.encode(*inputs)
        enc, st = eng.encoder_outputs()
    finally:
        eng.close()
    q = {'enc_out': enc}
    for n in range(d):
        q['h%d' % (n + 1)], q['c%d' % (n + 1)] = st[2 * n], st[2 * n + 1]
    return q


# ---------------------------------------------------------------------------------------------------------------------------
# decoder step

def build_step(case, seed=7, window=None):
    """cfg, float32 weights, and the step-0 inputs: line (R,), enc (lines,T,C), states [h1,c1,...], a (R,T), p_in (R,V).
    window: the attention's window width (ModelConfig.window; step_engine hands it to the device), None = the default 5.
    Row kinds by r % 8: 0 one-hot, 1 all zero (t' = 1), 2 spread near the start, 3 spread at the end (window partly off the line),
    4 empty window (t' > T + 4), 5-7 spread over three neighbours anywhere."""
    name, d, W, V, R, T, nl, steps = case
    cfg = ModelConfig(depth=d, width=W, voc_size=V) if window is None else ModelConfig(depth=d, width=W, voc_size=V, window=window)
    w = make_weights(cfg, emb_scale=4.0)
    rng = np.random.default_rng(seed)
    for k in w:
        if k.endswith('_b') or k in ('att_bUW', 'att_bv'):
            w[k] = (w[k] + rng.normal(size=w[k].shape) * 0.2).astype(np.float32)
    line = (np.arange(R) % nl).astype(np.int32)
    enc = (rng.normal(size=(nl, T, cfg.ctx_width)) * 0.5).astype(np.float32)
    states = [(rng.normal(size=(R, W)) * 0.5).astype(np.float32) for _ in range(2 * d)]
    logits = rng.normal(0, 2.0, (R, V))
    p_in = np.exp(logits - logits.max(axis=1, keepdims=True))
    p_in = (p_in / p_in.sum(axis=1, keepdims=True)).astype(np.float32)
    a = np.zeros((R, T), np.float32)
    kind = np.arange(R) % 8
    pos = rng.integers(0, T - 2, R)
    pos[kind == 2] = 0
    pos[kind == 3] = T - 3
    for k in range(3):
        a[np.arange(R), pos + k] = rng.random(R).astype(np.float32) + 0.1
    a[kind == 0] = 0
    a[kind == 0, pos[kind == 0]] = 1
    a[kind == 1] = 0
    a[kind == 4] = 0
    a[kind == 4, T - 1] = 1
    a[kind == 4, T - 2] = 0.6                                    # t' = T + 0.6 (T - 2) > T + 4
    s = a.sum(axis=1, keepdims=True)
    spread = kind >= 2
    spread &= kind != 4
    a[spread] /= s[spread]
    return cfg, w, (line, enc, states, a, p_in)


def oracle_step(cfg, w, line, enc, states, a, p_in, dtype, attention=None):
    """{probs, lm, h1, c1, ..., a} of one step of the oracle in `dtype` (rows in chunks); float64 decides the window in float32.
    attention: replaces oracle.model.attention for the call (mutations)."""
    wd = {k: np.asarray(v, dtype) for k, v in w.items()}
    encd = np.asarray(enc, dtype)
    u = encd @ wd['att_U']
    wdt = np.float32 if dtype == np.float64 else None
    m = OracleModel(cfg, wd)
    outs = []
    ctx = _patched(om_model, 'attention', attention) if attention else contextlib.nullcontext()
    with ctx, np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        for r0 in range(0, len(line), CHUNK):
            sl = slice(r0, r0 + CHUNK)
            st = [np.asarray(x[sl], dtype) for x in states] + [np.asarray(a[sl], dtype)]
            er = encd[line[sl]]
            p, ns = decoder_step(cfg, wd, np.asarray(p_in[sl], dtype), er, st, u=u[line[sl]], window_dtype=wdt)
            lm = lm_step(m, np.asarray(p_in[sl], dtype), er, st, window_dtype=wdt)
            outs.append([p, lm] + list(ns))
    cat = [np.concatenate([o[i] for o in outs]) for i in range(len(outs[0]))]
    q = {'probs': cat[0], 'lm': cat[1], 'a': cat[-1]}
    for n in range(cfg.depth):
        q['h%d' % (n + 1)], q['c%d' % (n + 1)] = cat[2 + 2 * n], cat[3 + 2 * n]
    return q


def next_inputs(cfg, q32):
    """The fp32 oracle's outputs as the next step's inputs (teacher forcing): states, a, p_in."""
    return [q32['%s%d' % (x, n + 1)] for n in range(cfg.depth) for x in 'hc'], q32['a'], q32['probs']


def device_step(eng, line, states, a, p_in):
    probs, lm, st = eng.decoder_step_lm(line, p_in, states, a)
    q = {'probs': probs, 'lm': lm, 'a': st[-1]}
    for n in range(eng.depth):
        q['h%d' % (n + 1)], q['c%d' % (n + 1)] = st[2 * n], st[2 * n + 1]
    return q


def step_engine(cfg, w, enc, arithmetic):
    from cor_asv_ann_amd.engine import HipEngine
    eng = HipEngine(cfg.depth, cfg.width, cfg.voc_size, window_width=cfg.window)
    eng.set_weights(w)
    eng.set_option('arithmetic', arithmetic)
    nl, T = enc.shape[:2]
    eng.set_encoder_outputs(enc, [np.zeros((nl, cfg.width), np.float32)] * (2 * cfg.depth))
    return eng


# ---------------------------------------------------------------------------------------------------------------------------
# mutations: mistakes a kernel could make, applied to the float64 oracle

@contextlib.contextmanager
def _patched(mod, name, value):
    old = getattr(mod, name)
    setattr(mod, name, value)
    try:
        yield
    finally:
        setattr(mod, name, old)


class _NumpyWithTanh(object):
    """numpy, except that tanh is off by `rel` (relative) on [lo, hi)."""
    def __init__(self, lo, hi, rel):
        self.lo, self.hi, self.rel = lo, hi, rel

    def __getattr__(self, k):
        return getattr(np, k)

    def tanh(self, x):
        y = np.tanh(x)
        return np.where((x >= self.lo) & (x < self.hi), y * (1 + self.rel), y)


def step_mutations(cfg, w, inputs, o64):
    """{name: float64 oracle step outputs} with one mistake each, on step 0 of a case (build_step)."""
    line, enc, states, a, p_in = inputs
    R, T = a.shape
    out = {}
    # (1) a window that loses its edge position on one row: the row whose edge weight is largest among those >= 1e-4
    edge = []
    for r in range(R):
        nz = np.nonzero(o64['a'][r])[0]
        if len(nz) > 1:
            for s in (nz[0], nz[-1]):
                if o64['a'][r, s] >= 1e-4:
                    edge.append((o64['a'][r, s], r, s))
    _, r0, s0 = min(edge)                                          # the smallest edge weight that still counts
    orig = om_model.attention

    def drop_edge(cfg_, w_, h, a_prev, enc_out, u, window_dtype=None):
        ctx, al = orig(cfg_, w_, h, a_prev, enc_out, u, window_dtype)
        al = al.copy()
        al[r0, s0] = 0
        al[r0] /= al[r0].sum()
        ctx = ctx.copy()
        ctx[r0] = (al[r0][:, None] * enc_out[r0]).sum(axis=0)
        return ctx, al
    assert R <= CHUNK                     # (one oracle call: attention sees the rows 0..R-1)
    out['window_edge_dropped'] = oracle_step(cfg, w, line, enc, states, a, p_in, np.float64, attention=drop_edge)
    # (2) one row's context rows (enc_out) or u rows taken from the neighbouring line
    r1 = R // 2
    nl = enc.shape[0]
    out['context_of_neighbour_line'] = _oracle_rows_from(cfg, w, inputs, r1, (line[r1] + 1) % nl, 'enc')
    out['u_of_neighbour_line'] = _oracle_rows_from(cfg, w, inputs, r1, (line[r1] + 1) % nl, 'u')
    # (3) one unit's forget-gate bias missing (top layer)
    w3 = dict(w)
    b = np.array(w['dec%d_b' % cfg.depth], copy=True)
    b[cfg.width + 3] = 0
    w3['dec%d_b' % cfg.depth] = b
    out['forget_bias_missing'] = oracle_step(cfg, w3, line, enc, states, a, p_in, np.float64)
    # (4) the last vocabulary entry of one row's fed-back distribution dropped
    p4 = np.array(p_in, copy=True)
    p4[r1, -1] = 0
    out['last_fed_back_entry_dropped'] = oracle_step(cfg, w, line, enc, states, a, p4, np.float64)
    # (5) tanh off by 1e-5 relative on one interval
    with _patched(om_model, 'np', _NumpyWithTanh(-2.0, 2.0, 1e-5)):
        out['tanh_off_1e-5_on_[-2,2)'] = oracle_step(cfg, w, line, enc, states, a, p_in, np.float64)
    return out


def _oracle_rows_from(cfg, w, inputs, r, other, what):
    """float64 oracle step where row r reads its enc rows ('enc') or its u rows ('u') from line `other`."""
    line, enc, states, a, p_in = inputs
    wd = {k: np.asarray(v, np.float64) for k, v in w.items()}
    e64 = np.asarray(enc, np.float64)
    er, ur = e64[line], (e64 @ wd['att_U'])[line]
    if what == 'enc':
        er[r] = e64[other]
    else:
        ur[r] = e64[other] @ wd['att_U']
    st = [np.asarray(x, np.float64) for x in states] + [np.asarray(a, np.float64)]
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        p, ns = decoder_step(cfg, wd, np.asarray(p_in, np.float64), er, st, u=ur, window_dtype=np.float32)
        # the LM has no context: unchanged by either mistake
        lm = lm_step(OracleModel(cfg, wd), np.asarray(p_in, np.float64), er, st, window_dtype=np.float32)
    q = {'probs': p, 'lm': lm, 'a': ns[-1]}
    for n in range(cfg.depth):
        q['h%d' % (n + 1)], q['c%d' % (n + 1)] = ns[2 * n], ns[2 * n + 1]
    return q


def encoder_mutations(cfg, w, x):
    """{name: float64 oracle encoder outputs} with one mistake: one unit's forget-gate bias missing (first forward layer), tanh off
    by 1e-5 relative on one interval."""
    w1 = dict(w)
    b = np.array(w['enc1_fw_b'], copy=True)
    b[cfg.width + 3] = 0
    w1['enc1_fw_b'] = b
    out = {'forget_bias_missing': oracle_encoder(cfg, w1, x, np.float64)}
    with _patched(om_model, 'np', _NumpyWithTanh(-2.0, 2.0, 1e-5)):
        out['tanh_off_1e-5_on_[-2,2)'] = oracle_encoder(cfg, w, x, np.float64)
    return out
