"""The part of the train step behind the gradients -- norm, clip decision, Adam update -- and the loss head at its clip edges,
against float64 (tests/test_update_bounds.py without a GPU, tests/test_gpu_update.py on the device, profiles/r10_update_error.txt).

1. The update as an elementwise function of what the device itself holds
------------------------------------------------------------------------
Around one mode-1 step the tests read w, m, v and the step count before, and g (the gradient buffers keep the step's gradients:
Adam scales them in registers), the returned norm gn and w', m', v' after.  `restate` is Keras 2.3 Adam with global-norm clipping
 in float64 on those float32 values and on the FLOAT32 values of the hyper-parameters (they are float32 variables in
Keras and float32 fields of casv_adam_params):

    b1 = float64(float32(beta1)), likewise b2, lr, eps, clipnorm          1 - b1, 1 - b2: exact in float32 (0.5 <= b < 1, Sterbenz)
    norm32 = float32(gn)
    scale  = clipnorm / norm32   if clipnorm > 0 and norm32 >= clipnorm, else 1
    g_s = g * scale
    m' = b1 * m + (1 - b1) * g_s
    v' = b2 * v + (1 - b2) * g_s^2
    t = step + 1,  lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t)
    w' = w - lr_t * m' / (sqrt(v') + eps)              with the DEVICE's m' and v', so that each quantity is tested on its own

Bounds (derived, not measured).  u = 2^-24 is float32's unit roundoff: a correctly rounded operation has relative error <= u; a
division or square root that is not correctly rounded is allowed 2 ulp = 4u.  k roundings in a row give at most
gamma(k) = (1 + u)^k - 1 (= k u to first order; 1 + 4u <= (1 + u)^4).  A fused multiply-add only removes roundings.  The float64
evaluation itself errs by a few 2^-53, and pow / sqrt in lr_t (float64 on the device too, 1 - b^t >= 1 - b >= 1e-3) by < 2^-40.

  scale   one division: 4 roundings' worth -- none when the step does not clip (scale is exactly 1).
  g_s     scale's 4 + one multiplication = 5  (ds = 5 when clipped, 0 otherwise)
  m'      term b1 m: its multiplication + the addition = 2;  term (1-b1) g_s: ds + multiplication + addition = ds + 2
          |m' - ref| <= gamma(2 + ds) (|b1 m| + |(1-b1) g_s|)                                  clipped 7u, unclipped 2u
  v'      term b2 v: 2;  term ((1-b2) g_s) g_s: 2 ds + two multiplications + the addition = 2 ds + 3
          |v' - ref| <= gamma(3 + 2 ds) (|b2 v| + |(1-b2) g_s^2|)                              clipped 13u, unclipped 3u
  w'      the update lr_t m' / (sqrt(v') + eps): lr_t rounded to float32 1, lr_t m' 1, sqrt 4, + eps 1, division 4 = 11, and one
          more for the denominator's error entering as 1 / (1 - 5u); then w - update is rounded once, relative to the result:
          |w' - ref| <= u (1 + 2u) |w'| + gamma(12) |lr_t m' / (sqrt(v') + eps)|
  The issue's constants were 8u, 12u and u + 12u; the count above differs for v' (13 against 12 when the step clips) and is tighter
  everywhere when it does not.  Absolute floors for products that underflow (flushed to zero at worst, 2^-126 each): 2^-120 on m'
  and v', and 2^-126 / eps <= 2^-100 on w'.

The norm: gn^2 against the float64 sum of squares of the g read back over the trained tensors, relative error <= 2^-40 (the device
accumulates in double; n 2^-53 is far below).  That sees a tensor left out, counted twice, a frozen one counted, float accumulation.

2. The clip decision: sessions on the same weights and batch, clipping off and clipnorm one float32 above, at and below float32(gn).

3. The loss head at its clip edges: the *saturated head* family (`saturated`), built by construction.  Every kernel and attention
tensor is zero; the top decoder layer's biases give i = 1/2, f = o = fl(sigmoid(30)) = 1, g = 0.2, every other bias is 0: the
encoder and the lower decoder layers hold h = c = 0, the top layer's c_u = 0.1 u and every unit of h_u is tanh(0.1 u).  E's rows are
multiples s_v e of one direction with sum(e) = 1, so logit_v(u) = s_v tanh(0.1 u): the last character has s = kappa, the others
+-0.02 kappa at most.  A row's target probability follows from (u, target) alone; the targets are picked from the float64 oracle's
table P[u, v] so that the classes below 1e-7 / inside / above 1 - 1e-7 alternate, each with a factor 8 to the thresholds (the tests
ask for 4).  kappa = 66 gives the mixed case: steps 1 and 2 are inside whatever the target, step 3 is below for every target but
the last character (which is too near the upper threshold there and is not used), later steps above or below by target.  (With
kappa = 80 only the last character was inside at step 2, at 1 - p = 9e-6; every gradient that reaches the top layer's R and K came
from those rows alone, as p - 1 with 1 % of float32 resolution: the fp32 oracle's "noise" on them was one rounding error, not a
sample, and a device 1 ulp off in p stood at 9.3 units.  At 66 rows with other targets, p - y of order 1, carry those gradients.)
kappa = 400 gives the all-clipped one.  Ragged lines: a zero-weight row with a valid target behind each line, -1 rows behind that.
"""
import functools

import numpy as np

from oracle import ModelConfig, make_weights, make_lines, weight_names
from oracle.train import forward_backward
from tests import grad_noise_cases as gn

U = 2.0 ** -24
NORM_REL = 2.0 ** -40


def gamma(k):
    return (1.0 + U) ** k - 1.0


# ------------------------------------------------------------------------------------------------------------------ part 1: cases
# (name, d, W, V, B, L, emb_scale, masks, flags, alternatives, frozen prefixes) as tests/grad_noise_cases.py
ALL_TOPOLOGIES = dict(residual_connections=True, deep_bidirectional_encoder=True, bridge_dense=True)
CASES = [('d2_w32', 2, 32, 40, 4, 9, 3.0, False, {}, 1, ()),
         ('d3_w128_b37_m', 3, 128, 40, 37, 7, 4.0, True, {}, 1, ()),
         ('w50_padded', 2, 50, 40, 4, 9, 4.0, True, {}, 1, ()),
         ('topologies_d3', 3, 64, 40, 6, 9, 4.0, True, ALL_TOPOLOGIES, 1, ()),
         ('frozen', 3, 64, 40, 6, 9, 4.0, True, {}, 1, ('enc1_', 'dec1_')),
         ('d8_w32', 8, 32, 40, 3, 5, 3.0, False, {}, 1, ()),
         ('d5_deep_bridge', 5, 32, 40, 3, 5, 3.0, True, dict(deep_bidirectional_encoder=True, bridge_dense=True), 1, ())]
BY_NAME = {c[0]: c for c in CASES}
# trained tensors a case must have (6 d + 9 plain; deep: 3 more per layer above the first; bridge: 4 per layer), MULTI_MAX = 48
MULTI_MAX = 48
TENSORS = {'d2_w32': 21, 'd3_w128_b37_m': 27, 'w50_padded': 21, 'topologies_d3': 27 + 6 + 12, 'frozen': 27 - 9, 'd8_w32': 57,
           'd5_deep_bridge': 39 + 12 + 20}
SECOND_LIST = ('d8_w32', 'd5_deep_bridge')

DEFAULT = dict(lr=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-7, clipnorm=5.0)
HYPERS = {'default': DEFAULT,
          'never_clips': dict(DEFAULT, clipnorm=1000.0),
          'clip_off_0': dict(DEFAULT, clipnorm=0.0),
          'clip_off_neg': dict(DEFAULT, clipnorm=-1.0),
          'other': dict(lr=3e-4, beta1=0.8, beta2=0.99, epsilon=1e-5, clipnorm=1.0)}
CLIPS = {'default': True, 'never_clips': False, 'clip_off_0': False, 'clip_off_neg': False, 'other': True}
STEPS = (0, 1, 9, 999, 99999, 10000000)         # the count BEFORE the step; at the last one both corrections are exactly 1


def trained(names, frozen):
    return [k for k in names if not (frozen and k.startswith(tuple(frozen)))]


def tensor_names(case):
    cfg = ModelConfig(depth=case[1], width=case[2], voc_size=case[3], **case[8])
    return [n for n, _ in weight_names(cfg)]


def seeded_moments(shapes, seed):
    """|m| log-uniform in [1e-12, 1e2] with random sign, v log-uniform in [1e-24, 1e4], 10 % exact zeros each (independently)."""
    rng = np.random.default_rng(seed)
    m, v = {}, {}
    for k, s in shapes.items():
        a = 10.0 ** rng.uniform(-12, 2, s) * rng.choice([-1.0, 1.0], s)
        b = 10.0 ** rng.uniform(-24, 4, s)
        m[k] = np.where(rng.random(s) < 0.1, 0.0, a).astype(np.float32)
        v[k] = np.where(rng.random(s) < 0.1, 0.0, b).astype(np.float32)
    return m, v


# ------------------------------------------------------------------------------------------------------------------ part 1: restatement
def f32(x):
    return float(np.float32(x))


def lr_t_of(hyper, t):
    b1, b2, lr = f32(hyper['beta1']), f32(hyper['beta2']), f32(hyper['lr'])
    return lr * np.sqrt(1.0 - b2 ** float(t)) / (1.0 - b1 ** float(t))


def scale_of(hyper, gnorm):
    """(scale, clipped) from the float32 values of clipnorm and the norm."""
    c, n32 = f32(hyper['clipnorm']), f32(gnorm)
    clipped = c > 0 and n32 >= c
    return (c / n32 if clipped else 1.0), clipped


def restate(w, m, v, g, gnorm, step, hyper, m_dev, v_dev):
    """One tensor: (m_ref, bound), (v_ref, bound), (w_ref, bound) in float64 (module docstring).  step: the count before the step."""
    w, m, v, g, m_dev, v_dev = (np.asarray(x, np.float64) for x in (w, m, v, g, m_dev, v_dev))
    b1, b2, eps = f32(hyper['beta1']), f32(hyper['beta2']), f32(hyper['epsilon'])
    scale, clipped = scale_of(hyper, gnorm)
    ds = 5 if clipped else 0
    gs = g * scale
    m1, m2 = b1 * m, (1.0 - b1) * gs
    v1, v2 = b2 * v, (1.0 - b2) * gs * gs
    upd = lr_t_of(hyper, step + 1) * m_dev / (np.sqrt(v_dev) + eps)
    w_ref = w - upd
    return ((m1 + m2, gamma(2 + ds) * (np.abs(m1) + np.abs(m2)) + 2.0 ** -120),
            (v1 + v2, gamma(3 + 2 * ds) * (np.abs(v1) + np.abs(v2)) + 2.0 ** -120),
            (w_ref, U * (1 + 2 * U) * np.abs(w_ref) + gamma(12) * np.abs(upd) + 2.0 ** -100))


def sumsq(g, names):
    return float(sum((np.asarray(g[k], np.float64) ** 2).sum() for k in names))


def check(before, after, g, gnorm, step, hyper, names):
    """Errors of one step in units of the bounds: {'norm', 'm', 'v', 'w'} (<= 1: within), 'moved' = elements with m = v = g = 0
    whose weight changed its bits, 'scale'.  before / after = (w, m, v) dicts; names: the trained tensors."""
    s = sumsq(g, names)
    out = {'norm': abs(gnorm * gnorm - s) / s / NORM_REL, 'm': 0.0, 'v': 0.0, 'w': 0.0, 'moved': 0, 'scale': scale_of(hyper, gnorm)[0]}
    for k in names:
        refs = restate(before[0][k], before[1][k], before[2][k], g[k], gnorm, step, hyper, after[1][k], after[2][k])
        for q, got, (ref, bound) in zip('mvw', (after[1][k], after[2][k], after[0][k]), refs):
            with np.errstate(invalid='ignore'):
                r = np.abs(np.asarray(got, np.float64) - ref) / bound
            out[q] = max(out[q], float(np.where(np.isfinite(r), r, np.inf).max()))
        still = (np.asarray(before[1][k]) == 0) & (np.asarray(before[2][k]) == 0) & (np.asarray(g[k]) == 0)
        a, b = np.asarray(after[0][k], np.float32), np.asarray(before[0][k], np.float32)
        out['moved'] += int((a.view(np.uint32) != b.view(np.uint32))[still].sum())
    return out


# ------------------------------------------------------------------------------------------------------------------ part 1: a float32 run and its mutations
MUTATIONS = ('sqrt_of_v_plus_eps', 'no_bias_correction', 't_off_by_one', 'v_from_unscaled_gradient', 'scale_after_moment_update',
             'norm_counts_frozen', 'norm_stops_at_48', 'beta2_double')


def simulate(w, m, v, g, step, hyper, names, mutation=None):
    """The update in float32 numpy, operation by operation as the restatement orders them: (gn, w', m', v') over `names` (the trained
    tensors, in list order; `g` may hold more).  mutation: one of MUTATIONS, a mistake an update could make."""
    assert mutation is None or mutation in MUTATIONS
    F = np.float32
    counted = list(names)
    if mutation == 'norm_counts_frozen':
        counted = list(g)
    if mutation == 'norm_stops_at_48':
        counted = counted[:MULTI_MAX]
    gnorm = float(np.sqrt(sumsq(g, counted)))
    b1, b2, eps, c = F(hyper['beta1']), F(hyper['beta2']), F(hyper['epsilon']), F(hyper['clipnorm'])
    one_b1, one_b2 = F(1) - b1, F(1) - b2
    t = step + (2 if mutation == 't_off_by_one' else 1)
    lr_t = F(hyper['lr']) if mutation == 'no_bias_correction' else F(lr_t_of(hyper, t))
    if mutation == 'beta2_double':      # 1 - beta2 and lr_t from the double 0.999, not from its float32 value
        one_b2 = F(1.0 - hyper['beta2'])
        lr_t = F(f32(hyper['lr']) * np.sqrt(1.0 - hyper['beta2'] ** float(t)) / (1.0 - f32(hyper['beta1']) ** float(t)))
    n32 = F(gnorm)
    scale = c / n32 if (c > 0 and n32 >= c) else F(1)
    w2, m2, v2 = {}, {}, {}
    for k in names:
        gk = np.asarray(g[k], F)
        gs = gk * scale
        if mutation == 'scale_after_moment_update':
            m2[k] = (b1 * m[k] + one_b1 * gk) * scale
        else:
            m2[k] = b1 * m[k] + one_b1 * gs
        gv = gk if mutation == 'v_from_unscaled_gradient' else gs
        v2[k] = b2 * v[k] + one_b2 * gv * gv
        den = np.sqrt(v2[k] + eps) if mutation == 'sqrt_of_v_plus_eps' else np.sqrt(v2[k]) + eps
        w2[k] = w[k] - lr_t * m2[k] / den
        assert m2[k].dtype == F and v2[k].dtype == F and w2[k].dtype == F
    return gnorm, w2, m2, v2


# ------------------------------------------------------------------------------------------------------------------ part 1: the device
def raw_read(eng, what, name):
    """A tensor as it crosses the C ABI, dead-unit padding included.  what: 'w' (after train_weights()), 'g', 'm', 'v'."""
    from cor_asv_ann_amd import _native as nv
    a = np.empty(eng.pshapes[name], np.float32)
    if what == 'w':
        nv.check(eng.lib.casv_get_weight(eng.handle, name.encode(), nv.ptr(a), a.size))
    elif what == 'g':
        nv.check(eng.lib.casv_train_get_gradient(eng.handle, name.encode(), nv.ptr(a), a.size))
    else:
        nv.check(eng.lib.casv_train_get_state(eng.handle, name.encode(), 'mv'.index(what), nv.ptr(a), a.size))
    return a


def padding_of(eng, name):
    """True where the tensor's padded form holds a dead unit's element."""
    return np.asarray(eng._pad_weight(name, np.ones(eng.shapes[name], np.float32))).reshape(eng.pshapes[name]) == 0


class Session(object):
    """One engine on a case's weights; step() runs one mode-1 step in a fresh training session and reads everything around it."""

    def __init__(self, case, deterministic, seed=4):
        from cor_asv_ann_amd.engine import HipEngine
        self.case = case
        self.cfg, self.w, self.inputs, self.batch = gn.build(case, seed)
        self.eng = HipEngine(case[1], case[2], case[3], **case[8])
        self.eng.set_option('deterministic', deterministic)
        self.frozen = tuple(case[10])
        self.names = trained(list(self.eng.shapes), self.frozen)

    def close(self):
        self.eng.close()

    def begin(self, hyper):
        self.eng.set_weights(self.w)
        self.eng.train_begin(frozen=self.frozen, **hyper)

    def read(self):
        m, v, step = self.eng.train_state()
        return (self.eng.train_weights(), m, v), step

    def step(self):
        """(before, after, g, gn, step before) of one mode-1 step of the current session."""
        before, step = self.read()
        _, gnorm = self.eng.train_step(*self.batch, mode=1)
        g = self.eng.train_gradients()
        after, step2 = self.read()
        assert step2 == step + 1
        return before, after, g, float(gnorm), step


# ------------------------------------------------------------------------------------------------------------------ part 3: saturated head
KAPPA = {'mixed': 66.0, 'all_clipped': 400.0}
LENS = (10, 7, 5, 9, 6, 8)
EPS = 1e-7
HEAD_CASES = [(kind, V, d) for kind in ('mixed', 'all_clipped') for V in (40, 65, 96) for d in (1, 2)]
HEAD_W = 32


def one_hot(idx, V):
    out = np.zeros(idx.shape + (V,), np.float32)
    b, t = np.nonzero(idx >= 0)
    out[b, t, idx[b, t]] = 1.0
    return out


def saturated_weights(cfg, kappa):
    W, V, d = cfg.width, cfg.voc_size, cfg.depth
    w = {k: np.zeros_like(a) for k, a in make_weights(cfg).items()}
    b = np.zeros(4 * W)
    b[W:2 * W] = 30.0                   # f = fl(sigmoid(30)) = 1
    b[2 * W:3 * W] = np.arctanh(0.2)    # g = 0.2, i = sigmoid(0) = 1/2: c grows by 0.1 a step
    b[3 * W:] = 30.0                    # o = 1
    w['dec%d_b' % d] = b.astype(np.float32)
    e = 1.0 + 0.25 * np.cos(np.arange(W))
    e /= e.sum()
    s = kappa * 0.02 * (((7 * np.arange(V)) % 11) - 5) / 5.0
    s[V - 1] = kappa                    # (V = 65: the one index of the second round of a 64-wide loop)
    w['E'] = (s[:, None] * e[None, :]).astype(np.float32)
    return w


def classes(p, factor=1.0):
    """-1 below 1e-7, 0 inside, +1 above 1 - 1e-7, each with `factor` to spare (on 1 - p at the upper one); -9 where none holds."""
    p = np.asarray(p, np.float64)
    out = np.full(p.shape, -9)
    out[p < EPS / factor] = -1
    out[(p > EPS * factor) & (1 - p > EPS * factor)] = 0
    out[1 - p < EPS / factor] = 1
    return out


def _forward(cfg, w, sidx, dec_in, dec_out, wts, dtype, want_grads):
    V = cfg.voc_size
    cast = lambda a: np.asarray(a, dtype)
    return forward_backward(cfg, {k: cast(a) for k, a in w.items()}, cast(one_hot(sidx, V)), cast(one_hot(dec_in, V)),
                            cast(one_hot(dec_out, V)), cast(wts), None, want_grads=want_grads, window_dtype=np.float32)


@functools.lru_cache(maxsize=None)
def saturated(kind, V, depth, weights=None):
    """cfg, weights, (sidx, dec_in, dec_out, wts) index arrays of a saturated-head case.  weights: None, or 'zero' for the same
    batch with every weight 0 (the regulariser's gradient alone)."""
    cfg = ModelConfig(depth=depth, width=HEAD_W, voc_size=V)
    w = saturated_weights(cfg, KAPPA[kind])
    B, Umax = len(LENS), max(LENS)
    _, sidx = make_lines(B, 6, 1, voc_size=V)
    # the float64 oracle's table P[u, v]: with zero kernels it depends on neither the line nor the targets
    blank = np.full((B, Umax), -1, np.int32)
    _, _, aux = _forward(cfg, w, sidx, blank, blank, np.zeros((B, Umax)), np.float64, False)
    P = aux['probs'][0]
    assert np.array_equal(aux['probs'], np.broadcast_to(P, aux['probs'].shape))
    cls = classes(P, 8.0)
    cycle = (0, 1, -1) if kind == 'mixed' else (1, -1)
    dec_out = np.full((B, Umax), -1, np.int32)
    wts = np.zeros((B, Umax), np.float32)
    for b, n in enumerate(LENS):
        for u in range(min(n + 1, Umax)):           # row n: a valid target with weight 0; behind it -1 rows
            for k in range(len(cycle)):
                cand = np.nonzero(cls[u] == cycle[(b + u + k) % len(cycle)])[0]
                if len(cand):
                    break
            dec_out[b, u] = cand[(5 * b + 3 * u) % len(cand)]
            wts[b, u] = 1.0 if u < n else 0.0
    dec_in = np.concatenate([np.full((B, 1), -1, np.int32), dec_out[:, :-1]], axis=1)
    if weights == 'zero':
        wts = np.zeros_like(wts)
    return cfg, w, (sidx, dec_in, dec_out, wts)


@functools.lru_cache(maxsize=None)
def head_oracle(kind, V, depth, dtype, weights=None):
    """(loss, norm, grads), loss_ce and the target probability of every row, of the oracle in `dtype` ('float32' / 'float64')."""
    cfg, w, (sidx, dec_in, dec_out, wts) = saturated(kind, V, depth, weights)
    loss, grads, aux = _forward(cfg, w, sidx, dec_in, dec_out, wts, np.dtype(dtype), True)
    grads = {k: np.asarray(a, np.float64) for k, a in grads.items()}
    pt = np.take_along_axis(aux['probs'], np.maximum(dec_out, 0)[:, :, None], axis=2)[:, :, 0]
    return (float(loss), float(np.sqrt(sumsq(grads, grads))), grads), float(aux['loss_ce']), np.asarray(pt, np.float64)


def head_device(cfg, w, batch, path, deterministic, modes=(0, 2)):
    """{mode: (loss, norm, grads)} of one step per mode on the device, no dropout masks."""
    from cor_asv_ann_amd.engine import HipEngine
    sidx, dec_in, dec_out, wts = batch
    eng = HipEngine(cfg.depth, cfg.width, cfg.voc_size)
    try:
        eng.set_weights(w)
        eng.set_option('persistent', -1 if path == 'fused' else 0)
        eng.set_option('fused_backward', 1 if path == 'fused' else 0)
        eng.set_option('deterministic', deterministic)
        eng.train_begin()
        out = {}
        for mode in modes:
            loss, norm = eng.train_step(sidx, None, dec_in, dec_out, wts, None, mode=mode)
            out[mode] = (float(loss), float(norm), eng.train_gradients() if mode == 2 else {})
        eng.train_end()
        return out
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------ part 3: the regulariser
def regulariser(E, dtype):
    """seq2seq.py:530-553 restated: sum((E[0] - stop_gradient(mean(E[1:], axis=0)))^2) + 0.01 sum((1 - sum(E^2, axis=1))^2) and its
    gradient with respect to E, everything in `dtype`."""
    E = np.asarray(E, dtype)
    d0 = E[0] - E[1:].mean(axis=0)
    norms = (E * E).sum(axis=1)
    one = E.dtype.type(1)
    loss = (d0 * d0).sum() + E.dtype.type(0.01) * ((one - norms) ** 2).sum()
    grad = (E.dtype.type(-0.04) * (one - norms))[:, None] * E
    grad[0] += E.dtype.type(2) * d0
    return float(loss), np.asarray(grad, np.float64)


def regulariser_ratios(E, loss_diff, loss_mode2, dE):
    """The device's regulariser loss (mode-2 loss - mode-0 loss; None: not compared) and gradient against the float64 restatement, in
    units of the float32 restatement's error (tests/grad_noise_cases.ratios); the loss difference's unit is floored at 2^-24 x the
    mode-2 loss as well, being a difference of two fp32-accurate numbers.  -> (loss ratio, (rms, max) ratios of dE)."""
    (l32, g32), (l64, g64) = regulariser(E, np.float32), regulariser(E, np.float64)
    r = gn.ratios((l64, 0.0, {'E': dE}), (l32, 0.0, {'E': g32}), (l64, 0.0, {'E': g64}))['E']
    if loss_diff is None:
        return 0.0, r
    unit = max(abs(l32 - l64), U * abs(l64), U * abs(loss_mode2))
    return abs(loss_diff - l64) / unit, r


REG_VARIANTS = ('unit_rows', 'times_0.05', 'times_128')


def regulariser_embedding(V, variant):
    """A random E with rows of norm exactly 1 (normalised in float64, then rounded), or that scaled by 0.05 or by 128."""
    E = np.random.default_rng(11).normal(size=(V, HEAD_W))
    E /= np.sqrt((E * E).sum(axis=1, keepdims=True))
    return (E * {'unit_rows': 1.0, 'times_0.05': 0.05, 'times_128': 128.0}[variant]).astype(np.float32)
