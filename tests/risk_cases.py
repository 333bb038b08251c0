"""The minimum-risk loss head (casv_train_step_risk / casv_debug_risk_rows) against its definition in numpy
(tests/test_risk_cases.py, tests/test_gpu_risk.py).

Definition (include/cor_asv_ann_hip.h): B = G * N lines, line b = g * N + i is candidate i of group g; cost (B), a negative cost =
not a member.  Per position (b,u) with t = target[b,u] >= 0 and w = weight[b,u] != 0, logp[b,u] = (x_t - m) - log(sum exp(x - m)):
    s_b   = sum over u ascending of (double)(w * logp[b,u])
    z_i   = alpha * s_i,  M = max z_i,  e_i = exp(z_i - M),  Z = sum e_i,  q_i = e_i / Z,  risk_g = sum q_i cost_i     (members, i ascending)
    inv   = 1 / max(groups with a member, 1),  c_i = alpha * q_i * (cost_i - risk_g) * inv,  loss = inv * sum risk_g
    dlogit[b,u][v] = c_b * w * ([v == t] - p_v)       (d risk_g / d s_i = c_i / inv, d logp / d x_v = [v == t] - p_v)
`head(dtype)` forms logp, p and dlogits in `dtype` and everything between s and c in float64, as the kernels do.

Two bounds.  (1) q and coef, the float64 part, against head(float64) fed the same float32 logp: |delta| <= COEF_RTOL * alpha * max
cost * inv -- four orders above the (N + 8) * 2^-53 of the operation count at N = 64, so a few ulp of a double exp do not matter,
while a dropped member or a wrong order moves a coefficient by parts in 10^2.  (2) the loss and dlogits in the project's noise
unit, as tests/soft_target_cases.py: C x max|f32 - f64|, floored at 2^-24 x max|f64|.  WRONG_HEADS are mistakes a kernel could
make; each misses the float64 head by at least 4 x one of the two bounds on at least one case (tests/test_risk_cases.py)."""
import numpy as np

# measured on an MI355X (profiles/risk_head_noise.txt): the largest ratio over all head cases and paddings is MEASURED_MAX_RATIO
# (the dlogits of V = 65, N = 3, G = 3, U = 1); C is twice that, rounded up
MEASURED_MAX_RATIO = 3.181
C = 7.0

COEF_RTOL = 1e-12

V_SIZES = (5, 64, 65, 96)              # below the lane count, equal to it, one over, Vp > V
N_SIZES = (1, 2, 3, 64)                # no choice, the smallest set, an odd one, every lane
HEAD_CASES = [(V, N, G, U) for V in V_SIZES for N in N_SIZES for G in (1, 3) for U in (1, 7)]
HEAD_CASES.append((640, 3, 3, 7))      # the page shape, once
HEAD_CASES.append((5, 64, 33, 4))      # 8448 rows: a second trip of the 2048-workgroup grid-stride loop
GROUP_KINDS = ('plain', 'nonmember_middle', 'all_nonmembers', 'equal_costs', 'one_zero', 'weight_0', 'weight_half', 'all_unscored',
               'low_target')
ALPHAS = (1.0, 0.25, 0.005)


def build(case):
    """x (B,U,V) float32, target (B,U) int32, weight (B,U) float32, cost (B) float32, alpha and the groups' kinds.  Group g is of
    kind GROUP_KINDS[(g + ordinal of the case) % 9], so that the one-group cases together see every kind; alpha rotates too.
    Lines have random lengths in [1, U], the positions behind them t = -1 with weight 0, as a vectorised batch."""
    V, N, G, U = case
    ordinal = HEAD_CASES.index(case) if case in HEAD_CASES else 0
    rng = np.random.default_rng(1000003 * V + 10007 * N + 101 * G + U)
    B = G * N
    x = (rng.normal(size=(B, U, V)) * 2.0).astype(np.float32)
    target = rng.integers(0, V, size=(B, U)).astype(np.int32)
    length = rng.integers(1, U + 1, size=B)
    target[np.arange(U)[None, :] >= length[:, None]] = -1
    cost = (rng.random(B) * 2.0).astype(np.float32)
    weight = (target >= 0).astype(np.float32)
    kinds = []
    for g in range(G):
        kind = GROUP_KINDS[(g + ordinal) % len(GROUP_KINDS)]
        kinds.append(kind)
        b0, mid = g * N, g * N + N // 2
        if kind == 'nonmember_middle':                  # (N = 1: the only line -- a group of non-members)
            cost[mid] = -1.0
        if kind == 'all_nonmembers':
            cost[b0:b0 + N] = -3.5                      # (any negative value)
        if kind == 'equal_costs':
            cost[b0:b0 + N] = 0.75
        if kind == 'one_zero':
            cost[b0:b0 + N] = (5.0 + 5.0 * rng.random(N)).astype(np.float32)
            cost[b0 + (N - 1) // 2] = 0.0
        if kind in ('weight_0', 'weight_half'):         # a scored position of the middle line
            weight[mid, (length[mid] - 1) // 2] = 0.0 if kind == 'weight_0' else 0.5
        if kind == 'all_unscored':                      # a member with s = 0
            target[b0 + N - 1] = -1
            weight[b0 + N - 1] = 0.0
        if kind == 'low_target':                        # p[t] ~ e^-40: far below any clip, still counted
            x[b0, 0, target[b0, 0]] = x[b0, 0].max() - 40.0
    return x, target, weight, cost, ALPHAS[ordinal % len(ALPHAS)], kinds


def row_logp(x, target, dtype=np.float64, pad=0, padded_sum=False):
    """(logp (B,U), p (B,U,V)) in `dtype`: logp = (x_t - m) - log(sum exp(x - m)), 0 where t < 0; p = exp(x - m) / sum.
    padded_sum: the mistake of counting `pad` padding columns of logit 0.0 in the row's maximum and sum."""
    dt = dtype
    x = np.asarray(x, dt)
    m = x.max(axis=2, keepdims=True)
    if padded_sum and pad:
        m = np.maximum(m, dt(0.0))
    e = np.exp(x - m)
    total = e.sum(axis=2, keepdims=True, dtype=dt)
    if padded_sum and pad:
        total = total + dt(pad) * np.exp(dt(0.0) - m)
    safe = np.where(target >= 0, target, 0)
    xt = np.take_along_axis(x, safe[:, :, None], axis=2)
    logp = ((xt - m) - np.log(total))[:, :, 0]
    return np.where(target >= 0, logp, dt(0.0)).astype(dt), (e / total).astype(dt)


def coefficients(logp, target, weight, cost, alpha, N, dtype=np.float64, wrong=None):
    """(loss, q (B), c (B)) in float64 from logp (B,U) in `dtype`: the part of the definition between logp and the coefficients."""
    dt = dtype
    target = np.asarray(target)
    logp = np.asarray(logp, dt)
    w = np.asarray(weight, dt)
    cost = np.asarray(cost, np.float64)
    B, U = target.shape
    G = B // N
    scored = (target >= 0) & (w != 0)
    if wrong == 'weight_0_counted':
        in_s, ws = target >= 0, np.where(w == 0, dt(1.0), w)
    else:
        in_s, ws = scored, w
    s = np.zeros(B, np.float32 if wrong == 's_float32' else np.float64)
    for u in range(U):                                  # (u ascending; the product in dt, the adds in double)
        s = s + np.where(in_s[:, u], (ws[:, u] * logp[:, u]).astype(dt), dt(0.0)).astype(s.dtype)
    s = s.astype(np.float64)
    # line of candidate i of group g
    line = (lambda g, i: i * G + g) if wrong == 'rows_transposed' else (lambda g, i: g * N + i)
    member = cost >= 0
    alpha = np.float64(alpha)
    groups = sum(1 for g in range(G) if any(member[line(g, i)] for i in range(N)))
    inv = 1.0 / max(G if wrong == 'empty_groups_counted' else groups, 1)
    q = np.zeros(B, np.float64)
    c = np.zeros(B, np.float64)
    total_risk = np.float64(0.0)
    with np.errstate(invalid='ignore', over='ignore'):
        for g in range(G):
            rows = [line(g, i) for i in range(N)]
            mem = [b for b in rows if member[b]]
            if not mem:
                continue
            in_z = rows if wrong == 'softmax_over_nonmembers' else mem
            z = {b: alpha * s[b] for b in in_z}
            M = -np.inf
            for b in in_z:
                M = z[b] if z[b] > M else M
            e = {b: np.exp(z[b] - M) for b in in_z}
            Z = np.float64(0.0)
            for b in in_z:
                Z = Z + e[b]
            risk = np.float64(0.0)
            for b in mem:
                q[b] = e[b] / Z
                risk = risk + q[b] * cost[b]
            for b in mem:
                if wrong == 'no_baseline':
                    c[b] = alpha * q[b] * cost[b] * inv
                elif wrong == 'alpha_missing':
                    c[b] = q[b] * (cost[b] - risk) * inv
                else:
                    c[b] = alpha * q[b] * (cost[b] - risk) * inv
            total_risk = total_risk + risk
    if wrong == 'sign_flipped':
        c = -c
    return float(inv * total_risk), q, c


def head(x, target, weight, cost, alpha, N, dtype=np.float64, wrong=None, pad=0, logp=None):
    """(loss, dlogits (B,U,V), q (B) float64, coef (B)) by the definition: logp, p, coef and dlogits in `dtype`, the sums between
    them in float64.  wrong: one of WRONG_HEADS; pad: the number of padding columns behind a row (they hold logit 0.0), which only
    the wrong head 'padding_in_sum' looks at; logp: (B,U) values to take in place of the head's own (the device's)."""
    dt = dtype
    target = np.asarray(target)
    w = np.asarray(weight, dt)
    cost = np.asarray(cost, np.float64)
    B, U, V = np.asarray(x).shape
    G = B // N
    own_logp, p = row_logp(x, target, dt, pad, wrong == 'padding_in_sum')
    logp = own_logp if logp is None else np.asarray(logp, dt)
    scored = (target >= 0) & (w != 0)
    loss, q, c = coefficients(logp, target, w, cost, alpha, N, dt, wrong)
    coef = c.astype(dt)
    onehot = np.zeros((B, U, V), dt)
    bb, uu = np.nonzero(target >= 0)
    onehot[bb, uu, target[bb, uu]] = 1
    d = (coef[:, None] * w)[:, :, None] * (onehot - p)
    d = np.where(scored[:, :, None], d, dt(0.0))
    return loss, d.astype(dt), q, coef


WRONG_HEADS = ('softmax_over_nonmembers', 'no_baseline', 'sign_flipped', 'alpha_missing', 'weight_0_counted', 'padding_in_sum',
               'empty_groups_counted', 'rows_transposed', 's_float32')


def coef_bound(cost, alpha, N):
    """The allowed error of q and coef given the same logp: COEF_RTOL * alpha * max cost * inv (q: COEF_RTOL alone would be the
    natural unit; the issue's one bound serves both, and alpha * max cost * inv <= 1 makes it the tighter)."""
    cost = np.asarray(cost, np.float64)
    G = len(cost) // N
    groups = sum(1 for g in range(G) if (cost[g * N:(g + 1) * N] >= 0).any())
    return COEF_RTOL * float(alpha) * max(float(cost.max()), 0.0) / max(groups, 1)


def coef_error(coef32, c64):
    """The error of float32 coefficients against float64 ones that the coefficient bound is asked of: per element |coef - c| less
    the 2^-24 |c| that rounding a double to float32 may move it by (the device stores float32: without this the format's own
    half ulp, 6e-8 |c|, would sit on a 1e-12 bound); the largest, never below 0.  A NaN is an infinite error."""
    a, r = np.asarray(coef32, np.float64), np.asarray(c64, np.float64)
    e = np.abs(a - r) - 2.0 ** -24 * np.abs(r)
    return float('inf') if np.isnan(e).any() else max(float(e.max()), 0.0)


def bounds(f32, f64, c=None, coef_floor=0.0):
    """The allowed error of (loss, dlogits): c x max|f32 - f64|, floored at 2^-24 x max|f64| (c = C by default).  coef_floor: the
    case's coefficient bound, a second floor under the unit of dlogits -- dlogit = c_b * w * ([v == t] - p_v) with |w|, |y - p| <= 1
    moves by what c_b may move by; without it a group of equal costs, whose coefficients are zero but for the last bits of
    cost - risk, has a unit of zero."""
    c = C if c is None else c
    out = []
    for a, r, floor in zip(f32[:2], f64[:2], (0.0, coef_floor)):
        a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
        unit = max(float(np.abs(a - r).max()), 2.0 ** -24 * max(float(np.abs(r).max()), 1e-30), floor)
        out.append(c * unit)
    return tuple(out)


def errors(got, f64):
    """max|got - f64| of (loss, dlogits); a NaN anywhere is an infinite error."""
    out = []
    for g, r in zip(got[:2], f64[:2]):
        e = np.abs(np.asarray(g, np.float64) - np.asarray(r, np.float64))
        out.append(float('inf') if np.isnan(e).any() else float(e.max()))
    return tuple(out)


_REFERENCES = {}


def reference(case):
    """(inputs, f64 head, f32 head) of a case, computed once and shared (the arrays are read-only)."""
    if case not in _REFERENCES:
        inputs = build(case)
        x, target, weight, cost, alpha, _ = inputs
        N = case[1]
        f64 = head(x, target, weight, cost, alpha, N, np.float64)
        f32 = head(x, target, weight, cost, alpha, N, np.float32)
        for a in inputs[:4] + f64[1:] + f32[1:]:
            a.setflags(write=False)
        _REFERENCES[case] = (inputs, f64, f32)
    return _REFERENCES[case]


# ---- the whole step: tests/grad_noise_cases.py's cases as G groups of N candidates ----
# name: (N, cost) -- d2_w32_b4_m is G = 2, N = 2; d3_w64_b8_m is G = 2, N = 4 with one line that is not a member
STEP_CASES = {'d2_w32_b4_m': (2, (0.0, 0.75, 0.4, 0.1)),
              'd3_w64_b8_m': (4, (0.0, 0.5, 1.25, 0.25, 0.0, -1.0, 0.6, 0.6))}
STEP_ALPHA = 0.5


def step_inputs(name):
    """(case, cfg, float32 weights, oracle inputs, device batch, N, cost float32) of a whole-step case."""
    from tests import grad_noise_cases as gn
    case = [c for c in gn.CASES if c[0] == name][0]
    cfg, w, inputs, batch = gn.build(case)
    N, cost = STEP_CASES[name]
    return case, cfg, w, inputs, batch, N, np.asarray(cost, np.float32)


def step_reference(cfg, w, inputs, N, cost, alpha, dtype, frozen=()):
    """((loss, norm, grads), (lowest, highest) target probability of the members' scored positions) of the oracle in `dtype`:
    oracle.train.forward_backward run forward, the coefficients from its own probabilities by `coefficients`, then forward_backward
    again with the per-position weights -c_b * w[b,u] times the count its normalisation divides by -- its clipped cross-entropy
    backward (P - Y) * weight / count is then this head's dlogits c_b * w * (Y - P) wherever the target probabilities lie inside (1e-7, 1 - 1e-7)."""
    from oracle.train import forward_backward
    enc_in, dec_in, dec_out, wts, masks = inputs
    cast = lambda a: np.asarray(a, dtype)
    m = None if masks is None else {'enc': [cast(x) for x in masks['enc']], 'dec': [cast(x) for x in masks['dec']], 'cell': cast(masks['cell'])}
    wd = {k: cast(v) for k, v in w.items()}
    _, _, aux = forward_backward(cfg, wd, cast(enc_in), cast(dec_in), cast(dec_out), cast(wts), m, want_grads=False,
                                 window_dtype=np.float32)
    y = np.asarray(dec_out)
    target = np.where(y.any(axis=2), y.argmax(axis=2), -1)
    pt = np.take_along_axis(np.asarray(aux['probs'], dtype), np.where(target >= 0, target, 0)[:, :, None], axis=2)[:, :, 0]
    scored = (target >= 0) & (np.asarray(wts) != 0)
    logp = np.where(target >= 0, np.log(np.where(target >= 0, pt, 1)), 0).astype(dtype)
    loss, _, c = coefficients(logp, target, wts, cost, alpha, N, dtype)
    per_position = (-c.astype(dtype)[:, None] * cast(wts)).astype(dtype)
    count = max(np.count_nonzero(per_position), 1)
    _, grads, aux2 = forward_backward(cfg, wd, cast(enc_in), cast(dec_in), cast(dec_out), (per_position * dtype(count)).astype(dtype), m,
                                      window_dtype=np.float32)
    grads = {k: np.asarray(g, np.float64) for k, g in grads.items() if not (frozen and k.startswith(tuple(frozen)))}
    norm = float(np.sqrt(sum((g ** 2).sum() for g in grads.values())))
    members = scored & (np.asarray(cost) >= 0)[:, None]
    return (float(loss + aux2['reg']), norm, grads), (float(pt[members].min()), float(pt[members].max()))
