"""The soft-target loss head (casv_train_step_soft / casv_debug_soft_ce_rows) against its definition in float64, in units of a
float32 numpy head's own rounding noise (tests/test_soft_target_cases.py, tests/test_gpu_soft_targets.py).

Definition (include/cor_asv_ann_hip.h): a row has V logits x, K slots (i_k, q_k) -- i_k = -1 empty, its q_k ignored -- and a weight
w; with p = softmax(x), ok_k = 1e-7 < p[i_k] < 1 - 1e-7 (the float32 constants of the kernel),
    loss     += w * inv_count * sum_k q_k * -log(clip(p[i_k], 1e-7, 1 - 1e-7))
    S         = sum_k q_k * ok_k
    dlogit[v] = (p_v * S - sum_{k: i_k == v} q_k * ok_k) * w * inv_count

Noise unit, as tests/grad_noise_cases.py: per output array (the loss, dlogits) the allowed error is C x max|f32 - f64|, floored at
2^-24 x max|f64|.  WRONG_HEADS are mistakes a kernel could make; each misses the float64 head by at least 4 x the bound on at least
one case (tests/test_soft_target_cases.py), so the bound cannot pass them."""
import numpy as np

LO = np.float32(1e-7)
HI = np.float32(1.0) - np.float32(1e-7)

# measured on an MI355X (profiles/soft_target_noise.txt): the largest ratio over all head cases, paddings, plain and ordered, is
# MEASURED_MAX_RATIO (the loss of V = 64, K = 64, R = 5); C is twice that, rounded up
MEASURED_MAX_RATIO = 3.027
C = 7.0

V_SIZES = (5, 64, 65, 96, 640)         # below the lane count, equal to it, one over, Vp > V, the page shape
R_SIZES = (1, 4, 5, 8197)              # a single row, a wave-tail row, a second trip of the grid-stride loop (4 x 2048 rows + 5)
HEAD_CASES = [(V, K, R) for V in V_SIZES for K in (1, 3, min(V, 64)) for R in R_SIZES]
ROW_KINDS = ('plain', 'empty_middle_sum_0.3', 'all_empty', 'weight_0', 'sum_2', 'entry_below_clip', 'entry_above_clip', 'weight_half')


def build(case):
    """logits (R,V) float32, soft_idx (R,K) int32, soft_q (R,K) float32, weight (R) float32, inv_count float32 and the rows' kinds.
    Row r is of kind ROW_KINDS[(r + ordinal of the case) % 8], so that the one-row cases together see every kind."""
    V, K, R = case
    ordinal = HEAD_CASES.index(case) if case in HEAD_CASES else 0
    rng = np.random.default_rng(1000003 * V + 1009 * K + R)
    x = (rng.normal(size=(R, V)) * 2.0).astype(np.float32)
    idx = np.empty((R, K), np.int32)
    q = np.empty((R, K), np.float32)
    w = np.ones((R,), np.float32)
    kinds = []
    for r in range(R):
        kind = ROW_KINDS[(r + ordinal) % len(ROW_KINDS)]
        kinds.append(kind)
        idx[r] = rng.permutation(V)[:K]
        mass = rng.random(K) + 0.05
        total = {'empty_middle_sum_0.3': 0.3, 'sum_2': 2.0}.get(kind, 1.0)
        if kind == 'empty_middle_sum_0.3':
            hole = K // 2                               # (K = 1: the only slot -- the row is all empty)
            keep = np.arange(K) != hole
            mass = np.where(keep, mass / max(mass[keep].sum(), 1e-30) * total, 0.7)        # an empty slot's mass is ignored
            idx[r, hole] = -1
        else:
            mass = mass / mass.sum() * total
        if kind == 'all_empty':
            idx[r] = -1                                 # (the masses stay: ignored)
        if kind == 'weight_0':
            w[r] = 0.0
        if kind == 'weight_half':
            w[r] = 0.5
        if kind == 'entry_below_clip':                  # p[i_0] ~ 1e-13: no gradient through that entry only
            x[r, idx[r, 0]] = x[r].max() - 30.0
        if kind == 'entry_above_clip':                  # p[i_0] > 1 - 1e-7, every other entry below 1e-7
            x[r, idx[r, 0]] = x[r].max() + 40.0
        q[r] = mass.astype(np.float32)
    inv_count = np.float32(1.0) / np.float32(max(int(np.count_nonzero(w)), 1))
    return x, idx, q, w, inv_count, kinds


def head(x, idx, q, w, inv_count, dtype=np.float64, wrong=None, pad=0):
    """(loss, dlogits (R,V)) by the definition, everything in `dtype` from the float32 inputs.  wrong: one of WRONG_HEADS; pad: the
    number of padding columns behind a row (they hold logit 0.0), which only the wrong head 'padding_in_sum' looks at."""
    dt = dtype
    x = np.asarray(x, dt); q = np.asarray(q, dt); w = np.asarray(w, dt)
    idx = np.asarray(idx)
    R, V = x.shape
    K = idx.shape[1]
    lo, hi = dt(LO), dt(HI)
    m = x.max(axis=1, keepdims=True)
    e = np.exp(x - m)
    total = e.sum(axis=1, keepdims=True, dtype=dt)
    if wrong == 'padding_in_sum':
        m = np.maximum(m, dt(0.0)) if pad else m
        e = np.exp(x - m)
        total = e.sum(axis=1, keepdims=True, dtype=dt) + dt(pad) * np.exp(dt(0.0) - m)
    p = e / total
    if wrong == 'empty_slot_as_index_0':
        idx = np.where(idx < 0, 0, idx)
    live = idx >= 0
    safe = np.where(live, idx, 0)
    pk = np.take_along_axis(p, safe, axis=1)                                    # (R,K)
    qk = np.where(live, q, dt(0.0))
    ok = ((pk > lo) & (pk < hi) & live).astype(dt)
    terms = (qk * -np.log(np.clip(pk, lo, hi))).sum(axis=1, dtype=dt)
    scale = w * dt(inv_count)
    if wrong == 'weight_0_row_has_gradient':
        gscale = np.where(w == 0, dt(1.0), w) * dt(inv_count)
    else:
        gscale = scale
    loss = float((terms * scale).astype(np.float64).sum())                     # (per row in dt, the rows added in double: as the kernel)
    qok = qk * ok
    S = qok.sum(axis=1, keepdims=True, dtype=dt)
    if wrong == 'S_ignores_ok':
        S = qk.sum(axis=1, keepdims=True, dtype=dt)
    sub = np.zeros((R, V), dt)
    rows = np.repeat(np.arange(R), K).reshape(R, K)
    if wrong == 'mass_at_slot_number':
        cols = np.broadcast_to(np.arange(K), (R, K))
        keep = live & (cols < V)
        np.add.at(sub, (rows[keep], cols[keep]), qok[keep])
    elif wrong == 'clip_rule_per_row':
        np.add.at(sub, (rows[live], safe[live]), qk[live])
    else:
        np.add.at(sub, (rows[live], safe[live]), qok[live])
    if wrong == 'clip_rule_per_row':                                            # the oracle's form: (p * sum q - y) * sum(y * inrange)
        d = (p * qk.sum(axis=1, keepdims=True, dtype=dt) - sub) * S * gscale[:, None]
    else:
        d = (p * S - sub) * gscale[:, None]
    return loss, d.astype(dt)


WRONG_HEADS = ('clip_rule_per_row', 'S_ignores_ok', 'empty_slot_as_index_0', 'padding_in_sum', 'weight_0_row_has_gradient',
               'mass_at_slot_number')


def bounds(f32, f64, c=None):
    """The allowed error of (loss, dlogits): c x max|f32 - f64|, floored at 2^-24 x max|f64| (c = C by default)."""
    c = C if c is None else c
    out = []
    for a, r in zip(f32, f64):
        a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
        unit = max(float(np.abs(a - r).max()), 2.0 ** -24 * max(float(np.abs(r).max()), 1e-30))
        out.append(c * unit)
    return tuple(out)


def errors(got, f64):
    """max|got - f64| of (loss, dlogits); a NaN anywhere is an infinite error."""
    out = []
    for g, r in zip(got, f64):
        e = np.abs(np.asarray(g, np.float64) - np.asarray(r, np.float64))
        out.append(float('inf') if np.isnan(e).any() else float(e.max()))
    return tuple(out)


_REFERENCES = {}


def reference(case):
    """(inputs, f64 head, f32 head) of a case, computed once and shared (the arrays are read-only)."""
    if case not in _REFERENCES:
        inputs = build(case)
        x, idx, q, w, inv_count, _ = inputs
        f64 = head(x, idx, q, w, inv_count, np.float64)
        f32 = head(x, idx, q, w, inv_count, np.float32)
        for a in inputs[:4] + (f64[1], f32[1]):
            a.setflags(write=False)
        _REFERENCES[case] = (inputs, f64, f32)
    return _REFERENCES[case]


def soften(dec_out_dense, probs, K=4, hard_share=0.55):
    """Normalised K-slot soft rows for a whole-step case: per scored position the hard target with `hard_share` and the K - 1
    likeliest other characters under `probs` (B,U,V) (a teacher's list) sharing the rest in proportion 3 : 2 : 1 ....  Returns
    (dense (B,U,V) float32 for the oracle, soft_idx (B,U,K) int32, soft_q (B,U,K) float32); an unscored position (zero row) has
    all-empty slots."""
    y = np.asarray(dec_out_dense)
    B, U, V = y.shape
    scored = y.any(axis=2)
    target = y.argmax(axis=2)
    rest = np.arange(K - 1, 0, -1, dtype=np.float64)
    rest = (1.0 - hard_share) * rest / rest.sum()
    dense = np.zeros((B, U, V), np.float32)
    soft_idx = np.full((B, U, K), -1, np.int32)
    soft_q = np.zeros((B, U, K), np.float32)
    for b, u in np.argwhere(scored):
        order = [v for v in np.argsort(-probs[b, u], kind='stable') if v != target[b, u]][:K - 1]
        soft_idx[b, u] = [target[b, u]] + order
        soft_q[b, u] = np.concatenate([[hard_share], rest]).astype(np.float32)
        soft_q[b, u, 0] += np.float32(1.0) - soft_q[b, u].sum(dtype=np.float32)       # (the float32 masses sum to 1)
        dense[b, u, soft_idx[b, u]] = soft_q[b, u]
    return dense, soft_idx, soft_q
