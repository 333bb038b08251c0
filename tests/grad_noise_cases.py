"""The train step's loss, norm and gradients against a float64 run of the oracle, in units of the fp32 oracle's own rounding noise
(tests/test_gpu_grad_noise.py, tests/test_grad_noise_bounds.py, profiles/gradient_noise.py).

For a case, o64 = oracle.train.forward_backward on float64 weights, inputs and masks, the attention window decided by the spec's
fp32 rule (window_dtype); o32 = the same in float32.  Per gradient
tensor, noise_rms = rms(o32 - o64) and noise_max = max|o32 - o64|; the device must stay within C_RMS x noise_rms (rms) and
C_MAX x noise_max (max), or 2^-24 x max|o64| where that is larger; the loss and the norm likewise with |o32 - o64|."""
import numpy as np

from oracle import ModelConfig, make_weights, make_lines, vectorize_lines
from oracle.decode import OracleModel
from oracle.train import forward_backward

# measured on an MI355X (profiles/r08_gradient_noise.txt): largest rms ratio 5.64, largest max ratio 3.99 (att_Wa / att_bUW, fused
# path): the constants are 2x those, rounded up
C_RMS, C_MAX = 12.0, 8.0
# att_bv's gradient is zero in exact arithmetic (adding a constant to every attention energy leaves the softmax unchanged): o32 - o64
# and device - o64 are both pure cancellation of O(1) terms, so their ratio says nothing (measured up to 102).  It keeps the absolute
# bound of tests/test_gpu_train.py instead (old_bound).
ZERO_GRADIENTS = ('att_bv',)


def within_old_bound(g, r, norm):
    """tests/test_gpu_train.py's per-tensor bound: max|g - r| < 2e-3 x max(max|r|, 1e-6 x norm) + 1e-7."""
    return float(np.abs(np.asarray(g, np.float64) - r).max()) < 2e-3 * max(float(np.abs(r).max()), 1e-6 * norm) + 1e-7


def excess(r):
    """How far the ratios of `r` (ratios()) go past the bound: max over quantities of ratio / constant (< 1: within)."""
    return max(max(a / C_RMS, b / C_MAX) for k, (a, b) in r.items() if k not in ZERO_GRADIENTS)


def _idx(a):
    return np.where(a.any(axis=2), a.argmax(axis=2), -1).astype(np.int32)


# (name, d, W, V, B, L, emb_scale, masks, flags, alternatives, frozen prefixes)
CASES = [('d%d_w%d_b%d%s' % (d, W, B, '_m' if mk else ''), d, W, V, B, L, es, mk, {}, 1, ())
         for d, W, V, B, L, es, mk in [(1, 32, 40, 4, 9, 3.0, False), (2, 32, 40, 4, 9, 3.0, True), (3, 64, 96, 8, 12, 6.0, True),
                                       (4, 64, 96, 6, 10, 8.0, False), (1, 20, 24, 3, 7, 3.0, True), (2, 50, 40, 4, 9, 4.0, True),
                                       (2, 96, 40, 5, 8, 4.0, True), (3, 160, 40, 3, 6, 4.0, False), (3, 128, 40, 37, 7, 4.0, True),
                                       (2, 256, 48, 5, 6, 4.0, False)]]
CASES += [('residual', 4, 64, 96, 6, 10, 8.0, True, dict(residual_connections=True), 1, ()),
          ('bridge', 3, 64, 40, 6, 9, 4.0, True, dict(bridge_dense=True), 1, ()),
          ('deep', 3, 96, 40, 5, 8, 4.0, True, dict(deep_bidirectional_encoder=True), 1, ()),
          ('confusion', 3, 64, 40, 6, 9, 4.0, True, {}, 2, ()),
          ('frozen', 3, 64, 40, 6, 9, 4.0, True, {}, 1, ('enc1_', 'dec1_'))]
# mid size: the encoder's weight gradients (M = 4W = 1024, N = W, K = B x 64) take the split and the ordered split forms
MID = ('mid_d2_w256_b512', 2, 256, 40, 512, 63, 4.0, True, {}, 1, ())
ALL = CASES + [MID]


def build(case, seed=4, source=None, window=None):
    """cfg, float32 weights, oracle inputs (enc_in, dec_in, dec_out, wts, masks) and the device batch of a case.
    source: None -- every source line has the targets' L characters and the end character; S -- the source lines have S characters
    and the end character (the targets keep L: the two lengths are separate), and about a third of them are shorter, the
    shortest of one character (where S = 1: the end character alone): the positions behind a line's end are zero rows for the oracle (the reference
    runs its LSTMs over them unmasked) and index -1 for the device.
    window: the attention's window width (ModelConfig.window; hand the same to `device`), None = the default 5."""
    name, d, W, V, B, L, es, with_masks, flags, A, frozen = case
    cfg = ModelConfig(depth=d, width=W, voc_size=V, **flags) if window is None else ModelConfig(depth=d, width=W, voc_size=V, window=window, **flags)
    w = make_weights(cfg, emb_scale=es)
    rng = np.random.default_rng(seed)
    for k in w:
        if k.endswith('_b') or k in ('att_bUW', 'att_bv'):
            w[k] = (w[k] + rng.normal(size=w[k].shape) * 0.2).astype(np.float32)
    om = OracleModel(cfg, w)
    src, sidx = make_lines(B, L if source is None else source, 1, voc_size=V)
    tgt, _ = make_lines(B, L, 2, voc_size=V)
    if B > 1:
        tgt[1] = tgt[1][:L // 2] + '\n'                     # ragged targets: padded steps have weight 0
    if source is not None:      # ragged sources, drawn apart from the jitter and the masks below (which stay what they are without)
        cut = np.random.default_rng(seed + 1)
        short = [b for b in range(1, B) if b % 3 == 2 or (B == 2 and b == 1)]
        for i, b in enumerate(short):
            src[b] = src[b][:min(1, source - 1) if i == 0 or source < 3 else int(cut.integers(1, source))] + '\n'
    enc_in, dec_in, dec_out, wts = vectorize_lines(om, src, tgt)
    if source is not None:
        sidx = _idx(enc_in)
    val = None
    if A > 1:                   # confusion network: two alternatives per position, 0.75 / 0.25
        alt = np.where(sidx >= 0, np.roll(sidx, 1, axis=1), -1)
        alt = np.where(alt >= 0, alt, sidx)
        enc_in = np.zeros(sidx.shape + (V,), np.float32)
        bb, tt = np.nonzero(sidx >= 0)
        enc_in[bb, tt, sidx[bb, tt]] += 0.75
        enc_in[bb, tt, alt[bb, tt]] += 0.25
        sidx = np.stack([sidx, alt], axis=2).astype(np.int32)
        val = np.stack([np.full(alt.shape, 0.75), np.full(alt.shape, 0.25)], axis=2).astype(np.float32)
    masks = None
    if with_masks:
        C = cfg.ctx_width
        keep = lambda shape: ((rng.random(shape) > 0.2) / 0.8).astype(np.float32)
        masks = {'enc': [keep(2 * W if (n == 0 or cfg.deep_bidirectional_encoder) else W) for n in range(d)],
                 'dec': [keep(W) for _ in range(d - 1)], 'cell': keep((B, W + C))}
    return cfg, w, (enc_in, dec_in, dec_out, wts, masks), (sidx, val, _idx(dec_in), _idx(dec_out), wts, masks)


def oracle(cfg, w, inputs, dtype, frozen=()):
    """(loss, norm, grads) of the oracle with everything in `dtype`; the norm over the trained tensors."""
    enc_in, dec_in, dec_out, wts, masks = inputs
    cast = lambda a: np.asarray(a, dtype)
    m = None if masks is None else {'enc': [cast(x) for x in masks['enc']], 'dec': [cast(x) for x in masks['dec']], 'cell': cast(masks['cell'])}
    loss, grads, _ = forward_backward(cfg, {k: cast(v) for k, v in w.items()}, cast(enc_in), cast(dec_in), cast(dec_out), cast(wts), m,
                                      window_dtype=np.float32)
    grads = {k: np.asarray(g, np.float64) for k, g in grads.items() if not (frozen and k.startswith(tuple(frozen)))}
    norm = float(np.sqrt(sum((g ** 2).sum() for g in grads.values())))
    return float(loss), norm, grads


def ratios(got, o32, o64):
    """{quantity: (rms ratio, max ratio)}: the error of `got` against o64 in units of the fp32 oracle's (rms, max) error, each unit
    floored at 2^-24 x max|o64|.  got, o32, o64 = (loss, norm, grads)."""
    out = {}
    items = [('loss', got[0], o32[0], o64[0]), ('norm', got[1], o32[1], o64[1])]
    items += [(k, got[2][k], o32[2][k], o64[2][k]) for k in sorted(o64[2])]
    for k, g, a, r in items:
        g, a, r = (np.asarray(x, np.float64) for x in (g, a, r))
        floor = 2.0 ** -24 * max(float(np.abs(r).max()), 1e-30)
        e, n = g - r, a - r
        rms = lambda x: float(np.sqrt(np.mean(x ** 2)))
        out[k] = (rms(e) / max(rms(n), floor), float(np.abs(e).max()) / max(float(np.abs(n).max()), floor))
    return out


def device(case, w, batch, path, deterministic, probe=None, window=None):
    """(loss, norm, grads) of one mode-2 train step on the device.  probe(eng): called behind the step, inside its session."""
    from cor_asv_ann_amd.engine import HipEngine
    name, d, W, V, B, L, es, with_masks, flags, A, frozen = case
    eng = HipEngine(d, W, V, **flags) if window is None else HipEngine(d, W, V, window_width=window, **flags)
    try:
        eng.set_weights(w)
        eng.set_option('persistent', -1 if path == 'fused' else 0)
        eng.set_option('fused_backward', 1 if path == 'fused' else 0)
        eng.set_option('deterministic', deterministic)
        eng.train_begin(frozen=frozen)
        loss, norm = eng.train_step(*batch, mode=2)
        grads = {k: g for k, g in eng.train_gradients().items() if not (frozen and k.startswith(tuple(frozen)))}
        if probe is not None:
            probe(eng)
        eng.train_end()
        return float(loss), float(norm), grads
    finally:
        eng.close()


def mutations(cfg, w, inputs, frozen=()):
    """{name: float64 oracle (loss, norm, grads)} of the case's inputs with one mistake a step could make: one target step's weight
    zeroed, one entry of the cell's dropout mask flipped (kept <-> dropped), one line's last real target step removed."""
    enc_in, dec_in, dec_out, wts, masks = inputs
    real = np.argwhere(np.asarray(wts) > 0)
    b, u = real[len(real) // 2]
    w1 = np.array(wts, copy=True); w1[b, u] = 0
    out = {'target_weight_zeroed': oracle(cfg, w, (enc_in, dec_in, dec_out, w1, masks), np.float64, frozen)}
    if masks is not None:
        m = {'enc': masks['enc'], 'dec': masks['dec'], 'cell': np.array(masks['cell'], copy=True)}
        c = m['cell']
        # (an entry of the y part whose input is not dropped already: [y | ctx], y behind the last decoder mask)
        i, j = c.shape[0] // 2, int(np.nonzero(masks['dec'][-1])[0][0]) if masks['dec'] else 0
        c[i, j] = 0.0 if c[i, j] != 0 else 1.0 / 0.8
        out['cell_mask_flipped'] = oracle(cfg, w, (enc_in, dec_in, dec_out, wts, m), np.float64, frozen)
    last = int(np.nonzero(np.asarray(wts)[0] > 0)[0].max())
    w2 = np.array(wts, copy=True); w2[0, last] = 0
    do = np.array(dec_out, copy=True); do[0, last] = 0
    out['last_step_removed'] = oracle(cfg, w, (enc_in, dec_in, do, w2, masks), np.float64, frozen)
    return out
