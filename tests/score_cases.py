"""Cases and references of the scoring head and of `score_targets` (csrc/train_kernels.hip: score_rows_kernel; csrc/score.hip:
casv_score_targets) -- helpers, no test.

  head64 / head32      the head restated in float64 on float32 logits, and in float32 numpy with the same formula
  HEAD_V, HEAD_SCALES  the head table (V x logit scale), head_case draws its rows; constructed_rows the rows built by hand
  MODEL_CASES          the model table, model_case builds a case by the recipe of tests/test_gpu_train.py (_train_step_case)
  oracles              fp32 and fp64 probabilities of a case (oracle.train.forward_backward, masks=None), computed once
  stepped              the teacher-forced forward pass restated step by step on oracle.model.encode / decoder_step: the reference for
                       the attention rows (forward_backward keeps them to itself); refused with residual_connections, where the
                       reference's inference decoder differs from its training graph
  MISTAKES             four wrong heads the GPU test's checks must catch (tests/test_score_cases.py)
"""
import functools

import numpy as np

from oracle import ModelConfig, make_weights, make_lines, vectorize_lines
from oracle.decode import OracleModel
from oracle.model import encode, decoder_step
from oracle.train import forward_backward

UNIT = 2.0 ** -24           # the bound's unit is UNIT * (|logp64| + 1): half an ulp of a float32 near 1, scaled with the result


# ------------------------------------------------------------------------------------------------------------------ the head
def _head(x, t, dt):
    """(logp, best, rank) of rows x (R,V) and targets t (R) in dtype dt; the issue's definition, row by row."""
    R, V = x.shape
    logp = np.zeros(R, dt)
    best = np.full(R, -1, np.int32)
    rank = np.full(R, -1, np.int32)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for r in range(R):
            row = x[r].astype(dt)
            m = np.max(row) if not np.isnan(row).any() else dt(np.nan)
            if not np.isfinite(m):
                logp[r] = np.nan
                continue
            best[r] = int(np.argmax(row == m))
            if 0 <= t[r] < V:
                xt = row[t[r]]
                logp[r] = (xt - m) - np.log(np.sum(np.exp(row - m), dtype=dt))
                rank[r] = int(np.count_nonzero(row > xt))
    return logp, best, rank


def head64(x, t):
    return _head(np.asarray(x, np.float32), np.asarray(t), np.float64)


def head32(x, t):
    return _head(np.asarray(x, np.float32), np.asarray(t), np.float32)


def units_or_inf(logp, logp64):
    """|logp - logp64| in the bound's units over the finite entries of logp64; inf where a NaN or an infinity is not where it belongs."""
    logp, logp64 = np.asarray(logp, np.float64), np.asarray(logp64, np.float64)
    fin = np.isfinite(logp64)
    with np.errstate(invalid='ignore'):
        out = np.abs(logp - logp64) / (UNIT * (np.abs(logp64) + 1.0))
    out[~fin] = np.where((logp[~fin] == logp64[~fin]) | (np.isnan(logp[~fin]) & np.isnan(logp64[~fin])), 0.0, np.inf)
    out[fin & ~np.isfinite(logp)] = np.inf
    return out


def units(logp, logp64):
    """... with every NaN and infinity where it belongs (asserted): the finite entries' errors."""
    out = units_or_inf(logp, logp64)
    assert np.isfinite(out).all()
    return out[np.isfinite(np.asarray(logp64, np.float64))]


HEAD_V = (2, 63, 64, 65, 255, 256, 257, 640, 4096)
HEAD_SCALES = (1.0, 10.0, 80.0)
HEAD_R = 64
PADS = (0.0, 3e38, np.inf, np.nan)


def head_case(V, s):
    """R rows of N(0, s) logits and their targets: 0, V - 1 and -1 among them."""
    rng = np.random.default_rng(1000 * V + int(s))
    x = (rng.standard_normal((HEAD_R, V)) * s).astype(np.float32)
    t = rng.integers(0, V, HEAD_R).astype(np.int32)
    t[0], t[1], t[2], t[3] = 0, V - 1, -1, -1
    return x, t


@functools.lru_cache(maxsize=None)
def e_np():
    """The float32-numpy head's largest error over the head table, in units: the reference's own float32 error."""
    worst = 0.0
    for V in HEAD_V:
        for s in HEAD_SCALES:
            x, t = head_case(V, s)
            worst = max(worst, float(units(head32(x, t)[0], head64(x, t)[0]).max()))
    return worst


def constructed_rows():
    """[(name, x (V,), t)]: the rows built by hand; their expected outputs are head64's, the named facts are asserted besides."""
    rng = np.random.default_rng(7)
    rows = []

    def base(V, lo=-3.0, hi=-1.0):
        return rng.uniform(lo, hi, V).astype(np.float32)
    rows.append(('all_equal', np.full(40, 1.5, np.float32), 7))
    for V, ties in ((40, (3, 9)), (40, (3, 9, 31)), (96, (5, 69)), (640, (69, 581)), (257, (256,))):
        for t in (ties[-1], 1):           # the target inside and outside the tie
            x = base(V)
            x[list(ties)] = 2.0
            rows.append(('tie_%d_%s_t%d' % (V, '_'.join(map(str, ties)), t), x, t))
    rows.append(('negative_only', base(40, -9.0, -2.0), 4))         # with pad_value 0 a read of the padding is the row's maximum
    rows.append(('negative_only_257', base(257, -9.0, -2.0), 256))
    for V, at in ((40, 0), (40, 39), (40, 17), (257, 256)):
        x = base(V); x[at] = np.nan
        rows.append(('nan_at_%d_of_%d' % (at, V), x, 3))
    x = base(40); x[11] = np.inf
    rows.append(('plus_inf', x, 11))
    rows.append(('all_minus_inf', np.full(40, -np.inf, np.float32), 2))
    x = base(40); x[6] = -np.inf
    rows.append(('minus_inf_at_target', x, 6))
    x = base(40); x[6] = -np.inf
    rows.append(('minus_inf_unscored', x, -1))
    return rows


# the four mistakes: name -> a head with that mistake, as (x, t, pad_value) -> (logp, best, rank) in float32
def _with_padding(x, t, pad):
    V = x.shape[1]
    Vp = (V + 31) // 32 * 32
    xp = np.full((x.shape[0], Vp), pad, np.float32)
    xp[:, :V] = x
    lp, b, r = head32(xp, t)
    return lp, b, r


def _rank_ge(x, t, pad):
    lp, b, r = head32(x, t)
    for i in range(len(t)):
        if r[i] >= 0:
            r[i] = int(np.count_nonzero(x[i] >= x[i, t[i]]))
    return lp, b, r


def _last_argmax(x, t, pad):
    lp, b, r = head32(x, t)
    for i in range(len(t)):
        if b[i] >= 0:
            b[i] = x.shape[1] - 1 - int(np.argmax(x[i, ::-1] == x[i].max()))
    return lp, b, r


def _clipped(x, t, pad):
    lp, b, r = head32(x, t)
    sc = r >= 0
    with np.errstate(divide='ignore'):
        lp[sc] = np.log(np.clip(np.exp(lp[sc]), np.float32(1e-7), np.float32(1 - 1e-7)))
    return lp, b, r


MISTAKES = {'padding_column_read': _with_padding, 'rank_counts_ties': _rank_ge, 'argmax_takes_the_last': _last_argmax,
            'loss_clip_on_logp': _clipped}


# ------------------------------------------------------------------------------------------------------------------ the model
# (d, W, V, B, L, emb_scale, flags, confusion-network input)
MODEL_CASES = [
    (1, 32, 40, 4, 9, 3.0, (), False),
    (2, 32, 40, 5, 9, 3.0, (), False),
    (3, 64, 96, 8, 12, 6.0, (), False),
    (2, 50, 40, 4, 9, 4.0, (), False),                     # dead-unit padding
    (3, 128, 40, 37, 7, 4.0, (), False),                   # rows across a 32-row block; persistent forms
    (2, 256, 48, 5, 6, 4.0, (), False),
    (2, 512, 40, 2, 6, 4.0, (), False),                    # two waves per attention row
    (2, 64, 257, 33, 20, 6.0, (), False),                  # V one past 256
    (2, 64, 640, 3, 11, 6.0, (), False),
    (4, 64, 96, 6, 10, 8.0, ('residual_connections', 'bridge_dense'), False),
    (3, 96, 40, 5, 8, 4.0, ('deep_bidirectional_encoder',), False),
    (2, 64, 40, 5, 9, 4.0, (), True),                      # A = 3, float values
]
BLOCK_CASE = MODEL_CASES[4]


def case_id(c):
    d, W, V, B, L, es, flags, conf = c
    return 'd%d_w%d_v%d_b%d_l%d%s%s' % (d, W, V, B, L, ''.join('_' + f.split('_')[0] for f in flags), '_conf' if conf else '')


IDS = [case_id(c) for c in MODEL_CASES]


def idx_of(a):
    return np.where(a.any(axis=2), a.argmax(axis=2), -1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def model_case(c):
    """cfg, weights, the batch in dense (oracle) and index (device) form; weights, biases, lines and the one shortened target as
    tests/test_gpu_train.py's _train_step_case draws them."""
    d, W, V, B, L, es, flags, conf = c
    cfg = ModelConfig(depth=d, width=W, voc_size=V, **{f: True for f in flags})
    w = make_weights(cfg, emb_scale=es)
    rng = np.random.default_rng(4)
    for k in w:
        if k.endswith('_b') or k in ('att_bUW', 'att_bv'):
            w[k] = (w[k] + rng.normal(size=w[k].shape) * 0.2).astype(np.float32)
    om = OracleModel(cfg, w)
    src, sidx = make_lines(B, L, 1, voc_size=V)
    tgt, _ = make_lines(B, L, 2, voc_size=V)
    tgt[1] = tgt[1][:L // 2] + '\n'
    enc_in, dec_in, dec_out, wts = vectorize_lines(om, src, tgt)
    enc_idx, enc_val = np.asarray(sidx, np.int32), None
    if conf:            # several weighted alternatives per position (tests/test_gpu_train.py, test_train_step_with_confidence_inputs)
        rng = np.random.default_rng(8)
        T, A = enc_in.shape[1], 3
        enc_idx = np.full((B, T, A), -1, np.int32)
        enc_val = np.zeros((B, T, A), np.float32)
        enc_idx[:, :, 0] = sidx
        enc_val[:, :, 0] = rng.uniform(0.3, 1.0, (B, T))
        alt = rng.random((B, T)) < 0.5
        enc_idx[:, :, 1] = np.where(alt, rng.integers(2, V, (B, T)), -1)
        enc_val[:, :, 1] = np.where(alt, rng.uniform(0.05, 0.5, (B, T)), 0.0)
        enc_idx[0, 2, 2] = 5; enc_val[0, 2, 2] = 0.1
        enc_idx[1, 3, :] = -1; enc_val[1, 3, :] = 0.0
        enc_in = np.zeros((B, T, V), np.float32)
        for b in range(B):
            for t in range(T):
                for a in range(A):
                    if enc_idx[b, t, a] >= 0:
                        enc_in[b, t, enc_idx[b, t, a]] += enc_val[b, t, a]
    return dict(cfg=cfg, w=w, flags={f: True for f in flags}, src=src, tgt=tgt, enc_in=enc_in, dec_in=dec_in, dec_out=dec_out, wts=wts,
                enc_idx=enc_idx, enc_val=enc_val, din=idx_of(dec_in), dout=idx_of(dec_out))


def stepped(cfg, w, enc_in, dec_in, window_dtype=None):
    """Teacher forcing on the reference's INFERENCE graph: one encode, then decoder_step per target position fed the one-hot dec_in
    row.  Returns (probs (B,U,V), attention rows (B,U,T)) in w's dtype."""
    if getattr(cfg, 'residual_connections', False):
        raise ValueError('the inference decoder has no residual sums: it does not restate the training graph (DESIGN.md section 0)')
    dt = w['E'].dtype
    outs = encode(cfg, w, enc_in)
    enc_out, states = outs[0], outs[1:]
    u = enc_out @ w['att_U']
    B, U, V = dec_in.shape
    probs = np.empty((B, U, V), dt)
    rows = np.empty((B, U, enc_in.shape[1]), dt)
    for t in range(U):
        p, states = decoder_step(cfg, w, dec_in[:, t].astype(dt), enc_out, states, u, window_dtype)
        probs[:, t], rows[:, t] = p, states[-1]
    return probs, rows


def _picks(P, dout):
    """best and rank of every position from a probability array, -1 where unscored (rank)."""
    best = P.argmax(axis=2).astype(np.int32)
    pt = np.take_along_axis(P, np.maximum(dout, 0)[:, :, None], axis=2)
    rank = np.where(dout >= 0, (P > pt).sum(axis=2), -1).astype(np.int32)
    return best, rank


@functools.lru_cache(maxsize=None)
def oracles(c):
    """What the device is compared with, computed once per case: the fp32 and fp64 oracles' probabilities, target probabilities,
    best and rank; `agree` = the positions where the two give the same best and (scored) the same rank; the stepped restatement's
    attention rows in fp64 (None with residual_connections)."""
    mc = model_case(c)
    cfg, w = mc['cfg'], mc['w']
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    args = (mc['enc_in'], mc['dec_in'], mc['dec_out'], mc['wts'])
    _, _, a32 = forward_backward(cfg, w, *args, None, want_grads=False)
    _, _, a64 = forward_backward(cfg, w64, *args, None, want_grads=False, window_dtype=np.float32)
    out = {'P32': a32['probs'], 'P64': a64['probs'], 'loss_ce32': a32['loss_ce']}
    dout = mc['dout']
    for k in ('32', '64'):
        P = out['P' + k]
        out['pt' + k] = np.take_along_axis(P, np.maximum(dout, 0)[:, :, None], axis=2)[:, :, 0]
        out['best' + k], out['rank' + k] = _picks(P, dout)
    out['agree'] = (out['best32'] == out['best64']) & (out['rank32'] == out['rank64'])
    out['rows64'] = None if cfg.residual_connections else stepped(cfg, w64, mc['enc_in'], mc['dec_in'], np.float32)[1]
    return out


def nll_of(logp, dout):
    """The lines' sums as the issue states them: a Python loop of double additions over the float32 logp, in the order of u."""
    nll, count = np.zeros(len(dout), np.float64), np.zeros(len(dout), np.int32)
    for b in range(len(dout)):
        acc = 0.0
        for u in range(dout.shape[1]):
            if dout[b, u] >= 0:
                acc += -float(logp[b, u])
                count[b] += 1
        nll[b] = acc
    return nll, count
