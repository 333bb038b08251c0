"""The bits the entry points between the C ABI and the step's phases hand back, one sha256 per line: run on two builds, the
outputs are equal iff the builds compute the same.

  (a) three mode-1 steps with "deterministic" = 1 through each of the five step entries (depth 2, width 48, V 37, B 4, T 9, U 7;
      soft K = 3; risk N = 2 with one negative cost; sampled ratio 0.5, 2 passes, pick 'sample'; the cut top_k 5, top_p 0.9):
      losses, norms, every weight, both Adam moments, and the sampled entries' mixes
  (b) score_targets and score_candidates (N = 2) on the same model: every output, dense and sparse alignments
  (c) the eight row-head test entries on fixed-seed logits, R = 5 (risk: G = 2, N = 2, U = 3), V = 37 (padding columns) and
      V = 64 (none), pad_value 3e38, soft_ce with ordered=True: every returned array

Fresh device buffers hold 0xFF bytes (CASV_POISON=1), so a byte no kernel writes is the same byte on every build.

    python profiles/entry_bits.py [--out FILE]
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault('CASV_POISON', '1')       # read once by the library, at its first allocation

DEPTH, WIDTH, V, B, T, U = 2, 48, 37, 4, 9, 7
STEP_ENTRIES = ('hard', 'soft', 'risk', 'sampled', 'sampled_cut')


def digest(*parts):
    h = hashlib.sha256()
    for p in parts:
        if isinstance(p, dict):
            for k in sorted(p):
                h.update(k.encode())
                h.update(np.ascontiguousarray(p[k]).tobytes())
        elif p is not None:
            h.update(np.ascontiguousarray(p).tobytes())
    return h.hexdigest()


def engine():
    from cor_asv_ann_amd.engine import HipEngine
    from cor_asv_ann_amd.synthetic import ModelConfig, make_weights
    eng = HipEngine(DEPTH, WIDTH, V)
    eng.set_weights(make_weights(ModelConfig(depth=DEPTH, width=WIDTH, voc_size=V)))
    return eng


def batch():
    rng = np.random.default_rng(11)
    enc = rng.integers(0, V, (B, T)).astype(np.int32)
    dec_in = rng.integers(0, V, (B, U)).astype(np.int32)
    dec_out = rng.integers(0, V, (B, U)).astype(np.int32)
    dec_out[1, U - 2:] = -1
    w = (dec_out >= 0).astype(np.float32)
    soft_idx = np.stack([rng.permutation(V)[:3] for _ in range(B * U)]).reshape(B, U, 3).astype(np.int32)
    soft_q = rng.random((B, U, 3)).astype(np.float32)
    cost = np.array([0.1, 0.7, -1.0, 0.4], np.float32)
    return enc, dec_in, dec_out, w, soft_idx, soft_q, cost


def step_bits(entry):
    enc, dec_in, dec_out, w, soft_idx, soft_q, cost = batch()
    eng = engine()
    eng.set_option('deterministic', 1)
    eng.train_begin()
    seen = []
    for i in range(3):
        if entry == 'hard':
            out = eng.train_step(enc, None, dec_in, dec_out, w, None, mode=1)
        elif entry == 'soft':
            out = eng.train_step_soft(enc, None, dec_in, soft_idx, soft_q, w, None, mode=1)
        elif entry == 'risk':
            out = eng.train_step_risk(enc, None, dec_in, dec_out, w, cost, 2, 1.0, None, mode=1, details=True)
        else:
            cut = dict(top_k=5, top_p=0.9) if entry == 'sampled_cut' else {}
            out = eng.train_step_sampled(enc, None, dec_in, dec_out, w, None, mode=1, ratio=0.5, seed=7, step_id=i, pick='sample',
                                         passes=2, **cut)
        seen += [np.float64(out[0]), np.float64(out[1])] + list(out[2:])
    m, v, step = eng.train_state()
    bits = digest(*seen, eng.train_weights(), m, v, np.int64(step))
    eng.train_end()
    eng.close()
    return bits


def score_bits():
    enc, dec_in, dec_out, _, _, _, _ = batch()
    eng = engine()
    out = {}
    for how in (True, 'sparse'):
        r = eng.score_targets(enc, None, dec_in, dec_out, want_align=how)
        out['score_targets align=%s' % how] = digest(*r[:5], *(r[5] if how == 'sparse' else (r[5],)))
        c_in = np.stack([dec_in, np.roll(dec_in, 1, axis=0)], axis=1)
        c_out = np.stack([dec_out, np.roll(dec_out, 1, axis=0)], axis=1)
        r = eng.score_candidates(enc, None, c_in, c_out, want_align=how)
        out['score_candidates N=2 align=%s' % how] = digest(*r[:5], *(r[5] if how == 'sparse' else (r[5],)))
    eng.close()
    return out


def row_bits(v):
    R, G, N, Us, pad = 5, 2, 2, 3, 3e38
    rng = np.random.default_rng(100 + v)
    x = (rng.standard_normal((R, v)) * 3).astype(np.float32)
    target = rng.integers(0, v, R).astype(np.int32)
    target[2] = -1
    gold, b, u = rng.integers(0, v, R).astype(np.int32), np.arange(R, dtype=np.int32), np.arange(R, dtype=np.int32) % 3
    uni = rng.random(R).astype(np.float32)
    soft_idx = np.stack([rng.permutation(v)[:3] for _ in range(R)]).astype(np.int32)
    soft_q = rng.random((R, 3)).astype(np.float32)
    weight = np.ones(R, np.float32)
    xr = (rng.standard_normal((G * N, Us, v)) * 3).astype(np.float32)
    tr = rng.integers(0, v, (G * N, Us)).astype(np.int32)
    wr = np.ones((G * N, Us), np.float32)
    cost = np.array([0.1, 0.7, -1.0, 0.4], np.float32)
    eng = engine()
    out = {
        'score_rows': eng.debug_score_rows(x, target, pad_value=pad),
        'alternatives_rows': eng.debug_alternatives_rows(x, 4, pad_value=pad),
        'sample_rows': eng.debug_sample_rows(x, temperature=0.8, top_k=5, seed=3, step=2, u=uni, pad_value=pad),
        'sample_cut_rows': eng.debug_sample_cut_rows(x, temperature=0.8, top_k=5, top_p=0.9, seed=3, step=2, u=uni, pad_value=pad),
        'soft_ce_rows': eng.debug_soft_ce_rows(x, soft_idx, soft_q, weight, 1.0 / R, pad_value=pad, want_grad=True, ordered=True),
        'risk_rows': eng.debug_risk_rows(xr, tr, wr, cost, N, 1.0, pad_value=pad, want_grad=True),
        'sched_rows': (eng.debug_sched_rows(x, gold, b, u, ratio=0.5, seed=3, step_id=1, pick='sample', temperature=0.8, pad_value=pad),),
        'sched_cut_rows': (eng.debug_sched_cut_rows(x, gold, b, u, ratio=0.5, seed=3, step_id=1, pick='sample', temperature=0.8, top_k=5,
                                                    top_p=0.9, pad_value=pad),),
    }
    eng.close()
    return {'%s V=%d' % (k, v): digest(*[np.asarray(a) for a in r]) for k, r in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    lines = ['step %s: %s' % (e, step_bits(e)) for e in STEP_ENTRIES]
    lines += ['%s: %s' % kv for kv in score_bits().items()]
    for v in (37, 64):
        lines += ['%s: %s' % kv for kv in row_bits(v).items()]
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
