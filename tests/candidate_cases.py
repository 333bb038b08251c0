"""Cases and references of `score_candidates` (csrc/score.hip: casv_score_candidates -- N candidate targets per source on one
encoder pass) -- helpers, no test.  The head, the bounds and the oracles' recipe are tests/score_cases.py's.

  CASES         the case table (d, W, V, Be, N, L, flags, confusion-network input) and what each row reaches
  case          cfg, weights, the Be sources and the Be * N candidates in index (device) form, and the replicated batch -- every
                source once per candidate -- in index and dense (oracle) form.  Sources make_lines(Be, L, 1, V), flat candidates
                make_lines(Be * N, L + 2, 2, V): U = L + 4 (L + 2 characters, the newline, the start position) != T = L + 1;
                candidate 1 is cut to L // 2 characters; where N >= 2 the last row is a padding candidate (all -1 on the device,
                zero one-hot rows and zero weight in the oracle)
  oracles       fp32 and fp64 oracles on the replicated batch (oracle.train.forward_backward), computed once per case
"""
import functools

import numpy as np

from oracle import ModelConfig, make_weights, make_lines, vectorize_lines
from oracle.decode import OracleModel
from oracle.train import forward_backward

from tests import score_cases as sc

# (d, W, V, Be, N, L, flags, confusion-network input)
CASES = [
    (1, 32, 40, 1, 1, 9, (), False),                       # the degenerate call
    (1, 64, 40, 2, 3, 9, (), False),                       # depth 1: no decoder layer below the cell, C = 2W
    (2, 32, 40, 2, 3, 9, (), False),                       # R = 6
    (2, 64, 40, 3, 11, 9, (), False),                      # R = 33: the decoder crosses a 32-row block, the encoder has one
    (3, 128, 40, 33, 2, 7, (), False),                     # encoder 2 blocks, decoder 3 blocks
    (2, 512, 40, 2, 2, 6, (), False),                      # two waves per attention row, rows_per_line 2
    (2, 256, 48, 2, 4, 6, (), False),                      # four attention rows per workgroup
    (2, 50, 40, 2, 3, 9, (), False),                       # dead-unit padding
    (2, 64, 257, 2, 17, 20, (), False),                    # V one past 256, R = 34
    (4, 64, 96, 3, 4, 10, ('residual_connections', 'bridge_dense'), False),        # replication behind the bridges
    (3, 96, 40, 2, 5, 8, ('deep_bidirectional_encoder',), False),                  # the decoder layer walks alone
    (2, 64, 40, 2, 3, 9, (), True),                        # A = 3 with float values
]
PLAIN = [c for c in CASES if not c[6] and not c[7]]


def case_id(c):
    d, W, V, Be, N, L, flags, conf = c
    return 'd%d_w%d_v%d_b%d_n%d_l%d%s%s' % (d, W, V, Be, N, L, ''.join('_' + f.split('_')[0] for f in flags), '_conf' if conf else '')


IDS = [case_id(c) for c in CASES]


@functools.lru_cache(maxsize=None)
def case(c):
    d, W, V, Be, N, L, flags, conf = c
    R = Be * N
    cfg = ModelConfig(depth=d, width=W, voc_size=V, **{f: True for f in flags})
    w = make_weights(cfg, emb_scale=4.0)
    rng = np.random.default_rng(4)
    for k in w:
        if k.endswith('_b') or k in ('att_bUW', 'att_bv'):
            w[k] = (w[k] + rng.normal(size=w[k].shape) * 0.2).astype(np.float32)
    om = OracleModel(cfg, w)
    src, sidx = make_lines(Be, L, 1, voc_size=V)
    tgt, _ = make_lines(R, L + 2, 2, voc_size=V)
    if R > 1:
        tgt[1] = tgt[1][:L // 2] + '\n'
    rep = [b for b in range(Be) for _ in range(N)]          # decoder row r = b * N + n reads source b
    enc_in, dec_in, dec_out, wts = vectorize_lines(om, [src[b] for b in rep], tgt)
    enc_idx, enc_val = np.asarray(sidx, np.int32), None
    if conf:            # several weighted alternatives per position, by score_cases.model_case's recipe on the Be sources
        rng = np.random.default_rng(8)
        T, A = enc_in.shape[1], 3
        enc_idx = np.full((Be, T, A), -1, np.int32)
        enc_val = np.zeros((Be, T, A), np.float32)
        enc_idx[:, :, 0] = sidx
        enc_val[:, :, 0] = rng.uniform(0.3, 1.0, (Be, T))
        alt = rng.random((Be, T)) < 0.5
        enc_idx[:, :, 1] = np.where(alt, rng.integers(2, V, (Be, T)), -1)
        enc_val[:, :, 1] = np.where(alt, rng.uniform(0.05, 0.5, (Be, T)), 0.0)
        enc_idx[0, 2, 2] = 5; enc_val[0, 2, 2] = 0.1
        enc_idx[1, 3, :] = -1; enc_val[1, 3, :] = 0.0
        one = np.zeros((Be, T, V), np.float32)
        for b in range(Be):
            for t in range(T):
                for a in range(A):
                    if enc_idx[b, t, a] >= 0:
                        one[b, t, enc_idx[b, t, a]] += enc_val[b, t, a]
        enc_in = one[rep]
    dec_in, dec_out, wts = dec_in.copy(), dec_out.copy(), np.array(wts, np.float32)
    if N >= 2:          # the last row: a padding candidate
        dec_in[-1] = 0; dec_out[-1] = 0; wts[-1] = 0
    din, dout = sc.idx_of(dec_in), sc.idx_of(dec_out)
    U, T = din.shape[1], enc_idx.shape[1]
    assert U == L + 4 and T == L + 1 and din.shape == dout.shape == (R, U)
    assert N < 2 or ((din[-1] == -1).all() and (dout[-1] == -1).all())
    return dict(cfg=cfg, w=w, flags={f: True for f in flags}, Be=Be, N=N, T=T, U=U,
                enc_idx=enc_idx, enc_val=enc_val, din=din.reshape(Be, N, U), dout=dout.reshape(Be, N, U),
                # the replicated batch: what score_targets takes, and what the oracle takes
                rep_idx=np.ascontiguousarray(enc_idx[rep]), rep_val=None if enc_val is None else np.ascontiguousarray(enc_val[rep]),
                rep_din=din, rep_dout=dout, enc_in=enc_in, dec_in=dec_in, dec_out=dec_out, wts=wts)


@functools.lru_cache(maxsize=None)
def oracles(c):
    """As score_cases.oracles, on the replicated batch: probabilities, target probabilities, best and rank of the fp32 and the fp64
    oracle, `agree` = the positions where the two give the same best and (scored) the same rank, the stepped restatement's
    attention rows in fp64 (None with residual_connections).  Computed once; nobody writes into it."""
    cc = case(c)
    cfg, w = cc['cfg'], cc['w']
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    args = (cc['enc_in'], cc['dec_in'], cc['dec_out'], cc['wts'])
    _, _, a32 = forward_backward(cfg, w, *args, None, want_grads=False)
    _, _, a64 = forward_backward(cfg, w64, *args, None, want_grads=False, window_dtype=np.float32)
    out = {'P32': a32['probs'], 'P64': a64['probs']}
    dout = cc['rep_dout']
    for k in ('32', '64'):
        P = out['P' + k]
        out['pt' + k] = np.take_along_axis(P, np.maximum(dout, 0)[:, :, None], axis=2)[:, :, 0]
        out['best' + k], out['rank' + k] = sc._picks(P, dout)
    out['agree'] = (out['best32'] == out['best64']) & (out['rank32'] == out['rank64'])
    out['rows64'] = None if cfg.residual_connections else sc.stepped(cfg, w64, cc['enc_in'], cc['dec_in'], np.float32)[1]
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
