"""Cases, references and bounds of sampling (csrc/sample_kernels.hip: sample_kernel; csrc/decode.hip: casv_decode_sample; csrc/debug_rows.hip:
casv_debug_sample_rows) -- helpers, no test.  Held on the CPU by tests/test_sample_cases.py, used on the device
by tests/test_gpu_sample.py.

  philox4x32_10 / uniform   the generator, written from the published algorithm (Salmon et al., SC'11), and the draw's uniform
  draw_rows                 the definition restated in float64 numpy on rows of logits (or of log-probabilities: w ~ p^(1/tau))
  left_out                  the ambiguity rule: a draw is not compared where u lies within delta of an interior boundary of the
                            float64 CDF or where the float32 and float64 candidates differ;
                            delta = max(C_MAX * max|CDF32 - CDF64| of the row, OLD_RT), the constants of tests/decode_noise_cases.py
  constructed_rows          the rows built by hand, with what the definition says of each
  MODEL_CASES, build_model  the model table; forced() runs the oracle along a given index sequence with one-hot inputs
  check_model               the GPU test's comparison of one sampling call with the oracle forced along the device's sequence
"""
import functools

import numpy as np

from oracle import ModelConfig, make_weights, make_lines
from oracle.model import encode, decoder_step
from tests.decode_noise_cases import C_MAX, OLD_RT, ratio

LEFT_OUT_CAP = 0.05         # at most this share of a case's draws may be left out
EOS = 1                     # the end-of-line index of the oracle's vocabulary

# ------------------------------------------------------------------------------------------------------------------ the generator
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Four output words of Philox4x32-10 for the counter (c0, c1, c2, c3) and the key (k0, k1); every word a uint64 array (or an
    int) holding 32 bits.  Round: (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)); the key
    goes up by (W0, W1) between rounds."""
    c = [np.asarray(x, np.uint64) & np.uint64(MASK) for x in counter]
    k = [np.asarray(x, np.uint64) & np.uint64(MASK) for x in key]
    for rnd in range(10):
        if rnd:
            k = [(k[0] + np.uint64(W0)) & np.uint64(MASK), (k[1] + np.uint64(W1)) & np.uint64(MASK)]
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]                 # (32 x 32 bits: no overflow of 64)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & np.uint64(MASK), (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & np.uint64(MASK)]
    return c


def uniform(seed, stream, n, s):
    """u = (o0 >> 8) * 2^-24 in [0, 1), o0 the first word for the counter (stream low, stream high, n, s) under the key (seed low,
    seed high); the arguments broadcast.  float32 (exact: 24 bits)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    stream = np.asarray(stream, np.int64).astype(np.uint64)
    o = philox4x32_10((stream & np.uint64(MASK), stream >> np.uint64(32), np.asarray(n, np.uint64), np.asarray(s, np.uint64)),
                      (seed & MASK, seed >> 32))[0]
    return ((o >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


KNOWN_ANSWERS = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                 ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                 ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


# ------------------------------------------------------------------------------------------------------------------ the definition
def draw_rows(x, u, tau=1.0, top_k=0, dt=np.float64):
    """The draw of every row of x (R,V) -- logits, or log-probabilities (w ~ p^(1/tau): the same weights) -- at the uniforms u (R).
    The candidates come from x as given (float32 logits: exact), the weights, prefix sums and logq are formed in dt.
    Returns dict(idx, logq, valid, cand (R,V) bool, cdf (R,V) normalised prefix sums over ALL indices (flat outside the candidates),
    w (R,V))."""
    x = np.asarray(x)
    R, V = x.shape
    tau = dt(np.float32(tau))
    cand = np.zeros((R, V), bool)
    cand[:, 1:] = True
    if 0 < top_k < V - 1:
        first = np.argsort(-x[:, 1:], axis=1, kind='stable')[:, :top_k] + 1      # x descending, the lower index among equals, -0 == +0
        cand[:] = False
        np.put_along_axis(cand, first, True, axis=1)
    xd = x.astype(dt)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        mc = np.where(cand, xd, -np.inf).max(axis=1) if V > 1 else np.full(R, -np.inf, dt)
        valid = ~np.isnan(xd).any(axis=1) & np.isfinite(mc)
        w = np.where(cand, np.exp((xd - mc[:, None]) / tau), dt(0)).astype(dt)
        w[~valid] = 0
        cdf = np.cumsum(w, axis=1, dtype=dt)
        Z = cdf[:, -1]
        target = np.asarray(u, dt) * Z
        above = cdf > target[:, None]
        last = V - 1 - (w[:, ::-1] > 0).argmax(axis=1)
        idx = np.where(above.any(axis=1), above.argmax(axis=1), last)
        idx[~valid] = 1
        rows = np.arange(R)
        logq = np.where(valid, (xd[rows, idx] - mc) / tau - np.log(Z), np.nan)
        cdfn = cdf / np.where(valid, Z, 1)[:, None]
    return dict(idx=idx.astype(np.int32), logq=logq, valid=valid, cand=cand, cdf=cdfn, w=w)


def left_out(u, d64, d32):
    """(left out (R) bool, distance (R) of u from the nearest interior boundary of the float64 CDF -- inf without one): the
    ambiguity rule of the module docstring on two draw_rows results of the same rows and uniforms."""
    u = np.asarray(u, np.float64)
    same = (d64['cand'] == d32['cand']).all(axis=1)
    c = np.asarray(d64['cdf'], np.float64)
    dev = np.abs(np.asarray(d32['cdf'], np.float64) - c).max(axis=1)
    delta = np.maximum(C_MAX * dev, OLD_RT)
    interior = d64['cand'] & (c > 0) & (c < 1)
    dist = np.where(interior, np.abs(u[:, None] - c), np.inf).min(axis=1)
    return ~same | (dist <= delta), dist


def onehot_rows(idx, valid, V):
    """The feedback rows (R,Vp): one-hot(idx) over Vp = V rounded up to 32 columns, all zero for an invalid row."""
    Vp = (V + 31) // 32 * 32
    out = np.zeros((len(idx), Vp), np.float32)
    out[np.nonzero(valid)[0], np.asarray(idx)[valid]] = 1.0
    return out


def constructed_rows():
    """[(name, x (V,), top_k, tau, facts)]: facts = dict of what the definition says of the row whatever u is: `valid`, `never` (indices
    that are never drawn), `only` (the indices that can be drawn)."""
    rng = np.random.default_rng(23)
    rows = []

    def base(V, lo=-3.0, hi=-1.0):
        return rng.uniform(lo, hi, V).astype(np.float32)
    # ties across the k-th place fall to the lower index: the group {38, 3, 31, 9} has two places left behind index 20
    x = base(40); x[20] = 4.0; x[[38, 3, 31, 9]] = 2.0
    rows.append(('tie_at_kth_40', x, 3, 1.0, dict(valid=True, only=(20, 3, 9))))
    x = base(96); x[50] = 4.0; x[[69, 5, 70, 20]] = 2.0
    rows.append(('tie_at_kth_96', x, 2, 2.0, dict(valid=True, only=(50, 5))))
    x = base(640); x[[69, 581, 133, 5, 639]] = 2.0; x[0] = 9.0          # (index 0 takes no place)
    rows.append(('tie_at_kth_640', x, 4, 1.0, dict(valid=True, only=(5, 69, 133, 581))))
    x = base(40); x[[4, 30]] = 0.0; x[[2, 9, 35]] = -0.0; x[x < 0] -= 5
    rows.append(('mixed_zeros_k3', x, 3, 1.0, dict(valid=True, only=(2, 4, 9))))
    x = np.full(40, -np.inf, np.float32); x[[7, 12, 33, 39]] = (-1.5, 0.25, -1.5, -4.0)
    rows.append(('minus_inf_members', x, 0, 1.0, dict(valid=True, only=(7, 12, 33, 39))))
    rows.append(('minus_inf_members_k8', x, 8, 1.0, dict(valid=True, only=(7, 12, 33, 39))))
    x = np.full(40, -np.inf, np.float32); x[0] = 1.0
    rows.append(('only_index_0_finite', x, 0, 1.0, dict(valid=False)))
    x = base(40); x[0] = 50.0
    rows.append(('index_0_largest', x, 0, 1.0, dict(valid=True, never=(0,))))
    for at in (0, 17, 39):
        x = base(40); x[at] = np.nan
        rows.append(('nan_at_%d' % at, x, 0, 1.0, dict(valid=False)))
    x = base(257); x[256] = np.nan
    rows.append(('nan_at_256_of_257', x, 5, 1.0, dict(valid=False)))
    x = base(40); x[11] = np.inf
    rows.append(('plus_inf', x, 0, 1.0, dict(valid=False)))
    rows.append(('all_equal', np.full(40, 1.5, np.float32), 0, 1.0, dict(valid=True, never=(0,))))
    rows.append(('all_equal_k5', np.full(40, 1.5, np.float32), 5, 1.0, dict(valid=True, only=(1, 2, 3, 4, 5))))
    rows.append(('all_minus_inf', np.full(40, -np.inf, np.float32), 0, 1.0, dict(valid=False)))
    rows.append(('v2', np.array([3.0, -1.0], np.float32), 0, 1.0, dict(valid=True, only=(1,))))
    rows.append(('cold', base(65), 0, 1e-3, dict(valid=True)))
    return rows


# the kernel alone: (V, R, top_k, tau, logit scale) -- every V, R, top_k and tau of the issue at least once; top_k 11 / 39 / 64 at V = 12 / 40 / 64, 65:
# ">= V - 1"; R = 1000: more than one workgroup and R % 4 == 0, 5 and 3: a partial last workgroup
KERNEL_CASES = [(12, 1, 0, 1.0, 2.0), (12, 5, 2, 0.5, 2.0), (12, 3, 11, 1.0, 2.0), (12, 4, 64, 2.0, 2.0),
                (40, 1000, 0, 1.0, 3.0), (40, 5, 1, 1.0, 3.0), (40, 4, 5, 0.5, 3.0), (40, 3, 39, 1e3, 3.0),
                (64, 5, 63, 1.0, 3.0), (64, 4, 64, 2.0, 3.0), (64, 3, 0, 1e-3, 3.0),
                (65, 5, 63, 0.5, 3.0), (65, 4, 64, 1.0, 3.0), (65, 1, 0, 1e3, 3.0),
                (96, 5, 2, 1.0, 4.0), (96, 37, 64, 2.0, 4.0), (96, 4, 0, 0.5, 10.0),
                (640, 5, 0, 1.0, 4.0), (640, 3, 64, 0.5, 4.0), (640, 4, 63, 1e-3, 4.0),
                (4096, 5, 0, 1.0, 3.0), (4096, 3, 64, 2.0, 3.0), (4096, 1, 1, 1.0, 3.0), (4096, 4, 63, 1e3, 3.0)]


def kernel_case(c):
    """Rows x (R,V) of a kernel case, their stream ids (beyond 2^32 among them), sample numbers, step and seed."""
    V, R, top_k, tau, scale = c
    rng = np.random.default_rng(100 * V + R + top_k)
    x = (rng.standard_normal((R, V)) * scale).astype(np.float32)
    streams = rng.integers(0, 2 ** 40, R).astype(np.int64)
    samples = rng.integers(0, 64, R).astype(np.int32)
    return x, streams, samples, int(rng.integers(0, 200)), int(rng.integers(0, 2 ** 63))


# ------------------------------------------------------------------------------------------------------------------ the model
# (name, depth, width, V, B, T, N, flags, confusion-network input, unequal lengths)
MODEL_CASES = [
    ('d1_w32_v12', 1, 32, 12, 4, 8, 16, (), False, False),
    ('d2_w64_v40_unequal', 2, 64, 40, 6, 12, 8, (), False, True),
    ('d2_w128_v96', 2, 128, 96, 4, 16, 8, (), False, False),
    ('d3_w64_v40_rows15', 3, 64, 40, 5, 10, 3, (), False, False),
    ('residual_d3_w64', 3, 64, 40, 4, 10, 4, ('residual_connections',), False, False),
    ('bridge_d2_w64', 2, 64, 40, 4, 10, 4, ('bridge_dense',), False, False),
    ('deep_d2_w64', 2, 64, 40, 4, 10, 4, ('deep_bidirectional_encoder',), False, False),
    ('confusion_d2_w64', 2, 64, 40, 4, 10, 4, (), True, False),
]
MODEL_IDS = [c[0] for c in MODEL_CASES]
FACADE_CASE = ('facade_d2_w64_v40', 2, 64, 40, 6, 10, 2, (), False, False)           # six lines of equal length, n = 2
BATCH_CASE = ('batch_d2_w64_v40', 2, 64, 40, 7, 10, 1, (), False, False)              # seven lines at one padded length
DRAWS = [(1.0, 0), (0.5, 5), (2.0, 0), (1.0, 1)]          # (tau, top_k)
CPU_CASES = [(MODEL_CASES[1], 1.0, 0), (MODEL_CASES[1], 0.5, 5), (MODEL_CASES[0], 2.0, 0), (MODEL_CASES[2], 1.0, 8)]      # the issue's table


@functools.lru_cache(maxsize=None)
def build_model(case):
    """cfg, float32 weights (biases drawn as tests/decode_noise_cases.py draws them), the oracle's input x (B,T,V) and the device's
    (idx, val), T = the padded length (the lines' characters and their end-of-line)."""
    name, d, W, V, B, L, N, flags, conf, unequal = case
    cfg = ModelConfig(depth=d, width=W, voc_size=V, **{f: True for f in flags})
    w = make_weights(cfg, emb_scale=4.0)
    rng = np.random.default_rng(3)
    for k in w:
        if k.endswith('_b') or k in ('att_bUW', 'att_bv'):
            w[k] = (w[k] + rng.normal(size=w[k].shape) * 0.2).astype(np.float32)
    _, sidx = make_lines(B, L - 1, 5, voc_size=V)                  # (B, L): L - 1 characters and the end-of-line
    sidx = np.array(sidx, np.int32)
    if unequal:
        for b in range(B):
            n = L - 1 - (b * 2) % (L // 2)
            sidx[b, n] = EOS
            sidx[b, n + 1:] = -1
    x = np.zeros(sidx.shape + (V,), np.float32)
    bb, tt = np.nonzero(sidx >= 0)
    if not conf:
        x[bb, tt, sidx[bb, tt]] = 1.0
        return dict(cfg=cfg, w=w, x=x, idx=sidx, val=None, flags={f: True for f in flags}, N=N)
    alt = np.where(sidx >= 0, np.roll(sidx, 1, axis=1), -1)        # confusion network: two alternatives, 0.75 / 0.25
    alt = np.where(alt >= 0, alt, sidx)
    x[bb, tt, sidx[bb, tt]] += 0.75
    x[bb, tt, alt[bb, tt]] += 0.25
    val = np.stack([np.full(alt.shape, 0.75), np.full(alt.shape, 0.25)], axis=2).astype(np.float32)
    return dict(cfg=cfg, w=w, x=x, idx=np.stack([sidx, alt], axis=2).astype(np.int32), val=val, flags={f: True for f in flags}, N=N)


@functools.lru_cache(maxsize=None)
def _encoded(case, dtype):
    mc = build_model(case)
    wd = {k: np.asarray(v, dtype) for k, v in mc['w'].items()}
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        outs = encode(mc['cfg'], wd, np.asarray(mc['x'], dtype))
    return wd, outs[0], outs[1:], outs[0] @ wd['att_U']


def forced(case, seq, dtype, follow=None):
    """The oracle in `dtype` (float64: the window decided in float32, as tests/decode_noise_cases.py) along the index sequence
    seq (B,N,S): row b * N + n starts from line b's encoder states and is fed the one-hot row of seq[b, n, s - 1] at step s > 0
    (zeros at step 0).  follow(s, p (R,V)) -> (R) indices, if given, decides the sequence instead (seq: its shape only).
    Returns (P (R,S,V), alignment rows (R,S,T), the sequence (R,S))."""
    mc = build_model(case)
    cfg = mc['cfg']
    wd, enc, states, u = _encoded(case, dtype)
    B, N, S = np.shape(seq)
    R, V = B * N, cfg.voc_size
    line = np.repeat(np.arange(B), N)
    enc, u, states = enc[line], u[line], [s[line] for s in states]
    P, A = np.empty((R, S, V), dtype), np.empty((R, S, enc.shape[1]), dtype)
    out = np.array(seq, np.int64).reshape(R, S)
    p_in = np.zeros((R, V), dtype)
    wdt = np.float32 if dtype == np.float64 else None
    for s in range(S):
        p, states = decoder_step(cfg, wd, p_in, enc, states, u=u, window_dtype=wdt)
        P[:, s], A[:, s] = p, states[-1]
        if follow is not None:
            out[:, s] = follow(s, p)
        p_in = np.zeros((R, V), dtype)
        p_in[np.arange(R), out[:, s]] = 1
    return P, A, out


def _logs(P):
    with np.errstate(divide='ignore'):
        return np.log(np.asarray(P, np.float64))


def lengths(seq):
    """Steps up to and including the first end-of-line of every row of seq (R,S); S without one."""
    hit = seq == EOS
    return np.where(hit.any(axis=1), hit.argmax(axis=1) + 1, seq.shape[1]).astype(np.int32)


def reference_run(case, tau, top_k, seed, S=None, streams=None):
    """The reference sampler alone: o64 draws its own sequence (streams default to the line numbers), o32 is forced along it.
    Returns what compare_draws needs and the sequence."""
    mc = build_model(case)
    B, N = mc['x'].shape[0], mc['N']
    S = S or 2 * mc['x'].shape[1]
    streams = np.arange(B) if streams is None else np.asarray(streams)
    U = uniform(seed, np.repeat(streams, N)[:, None], np.tile(np.arange(N), B)[:, None], np.arange(S)[None, :])

    def follow(s, p):
        return draw_rows(_logs(p), U[:, s], tau, top_k)['idx']
    P64, A64, seq = forced(case, np.zeros((B, N, S)), np.float64, follow)
    P32, A32, _ = forced(case, seq.reshape(B, N, S), np.float32)
    return dict(P64=P64, P32=P32, A64=A64, A32=A32, U=U, seq=seq)


def compare_draws(ref, seq, tau, top_k, reported):
    """Over the reported steps (R,S bool) of the sequence seq (R,S) both oracles were forced along: (draws, left out, mismatches
    outside the margin between seq and the float64 pick, o32/o64 disagreements outside the margin, the smallest delta at which
    every draw of seq would have matched)."""
    R, S = seq.shape
    n = out = wrong = disagree = 0
    need = 0.0
    for s in range(S):
        d64 = draw_rows(_logs(ref['P64'][:, s]), ref['U'][:, s], tau, top_k)
        d32 = draw_rows(_logs(ref['P32'][:, s]), ref['U'][:, s], tau, top_k)
        lo, dist = left_out(ref['U'][:, s], d64, d32)
        rep = reported[:, s]
        n += int(rep.sum())
        out += int((rep & lo).sum())
        miss = rep & (seq[:, s] != d64['idx'])
        wrong += int((miss & ~lo).sum())
        disagree += int((rep & ~lo & (d32['idx'] != d64['idx'])).sum())
        same = (d64['cand'] == d32['cand']).all(axis=1)
        if (miss & same).any():
            need = max(need, float(dist[miss & same].max()))
        if (miss & ~same).any():
            need = np.inf                     # (no delta explains a draw from other candidates)
    return n, out, wrong, disagree, need


def left_out_mask(ref, tau, top_k):
    """(R,S) bool: the draws the ambiguity rule leaves out, along the sequence both oracles of `ref` were forced along."""
    S = ref['U'].shape[1]
    return np.stack([left_out(ref['U'][:, s], draw_rows(_logs(ref['P64'][:, s]), ref['U'][:, s], tau, top_k),
                              draw_rows(_logs(ref['P32'][:, s]), ref['U'][:, s], tau, top_k))[0] for s in range(S)], axis=1)


def check_model(case, got, tau, top_k, seed, streams=None, align=None, sparse=None):
    """One sampling call's results got = (idx, logp, logq (B,N,S), length (B,N)) against the oracle forced along the DEVICE's
    sequence: at every reported step the index is the reference's pick unless left out, at most LEFT_OUT_CAP of the draws are left
    out, exp(logp) stays within C_MAX units of o32's own relative error from o64, logq within the same of the reference's, the
    alignment rows (align (B,N,S,T) dense, sparse (lo, w)) within C_MAX units absolutely, and length is the first end-of-line.
    Returns the figures."""
    idx, logp, logq, length = got[:4]
    B, N, S = idx.shape
    R = B * N
    seq = idx.reshape(R, S).astype(np.int64)
    assert (seq >= 1).all() and (seq < build_model(case)['cfg'].voc_size).all()
    assert np.array_equal(length.reshape(R), lengths(seq))
    reported = np.arange(S)[None, :] < length.reshape(R, 1)
    streams = np.arange(B) if streams is None else np.asarray(streams)
    U = uniform(seed, np.repeat(streams, N)[:, None], np.tile(np.arange(N), B)[:, None], np.arange(S)[None, :])
    P64, A64, _ = forced(case, idx, np.float64)
    P32, A32, _ = forced(case, idx, np.float32)
    ref = dict(P64=P64, P32=P32, U=U)
    n, out, wrong, _, need = compare_draws(ref, seq, tau, top_k, reported)
    rows, steps = np.nonzero(reported)
    p64, p32 = P64[rows, steps, seq[rows, steps]], P32[rows, steps, seq[rows, steps]]
    r_p = ratio(np.exp(logp.reshape(R, S)[rows, steps].astype(np.float64)), p32, p64, rel=True)
    q64 = np.empty((R, S))
    for s in range(S):
        d64 = draw_rows(_logs(P64[:, s]), U[:, s], tau, top_k)
        q64[:, s] = np.where(seq[:, s] == d64['idx'], d64['logq'], np.nan)          # (where the device drew the reference's pick)
    figures = dict(draws=n, left_out=out, wrong=wrong, need=need, logp=r_p, ref=ref, reported=reported)
    ok = reported & ~np.isnan(q64)
    figures['logq'] = float(np.abs(logq.reshape(R, S)[ok] - q64[ok]).max(initial=0.0))
    if align is not None:
        figures['align'] = ratio(align.reshape(R, S, -1)[rows, steps], A32[rows, steps], A64[rows, steps])
        assert np.array_equal(np.isnan(align.reshape(R, S, -1)[rows, steps]), np.isnan(A32[rows, steps]))
    if sparse is not None:
        lo, w = sparse[0].reshape(R, S), sparse[1].reshape(R, S, -1)
        T = A64.shape[2]
        dense = np.zeros((R, S, T + w.shape[2]), np.float32)
        for r, s in zip(rows, steps):
            if lo[r, s] < 0:
                dense[r, s] = np.nan
            else:
                dense[r, s, lo[r, s]:lo[r, s] + w.shape[2]] = w[r, s]
        figures['sparse'] = ratio(dense[rows, steps][:, :T], A32[rows, steps], A64[rows, steps])
    return figures
