"""Object wrapper over the C ABI (include/cor_asv_ann_hip.h): numpy in, numpy out.

This is plumbing between the `Sequence2Sequence` facade and the HIP library; all arithmetic of
the hot path happens in the library's kernels.
"""
import ctypes
from ctypes import byref, c_double, c_int64, c_void_p

import numpy as np

from . import _native as nv


def weight_shapes(depth, width, voc_size, bridge_dense=False, deep_bidirectional_encoder=False):
    """Ordered {name: shape} of the model's tensors in Keras layout (layer creation
    order of seq2seq.py:239-350 and attention.py:598-609; the bridge_dense layers of seq2seq.py:299-301 last)."""
    d, W, V = depth, width, voc_size
    deep = bool(deep_bidirectional_encoder)
    C = 2 * W if (d == 1 or deep) else W
    shapes = {'E': (V, W)}
    for direction in ('fw', 'bw'):
        shapes['enc1_%s_K' % direction] = (W, 4 * W)
        shapes['enc1_%s_R' % direction] = (W, 4 * W)
        shapes['enc1_%s_b' % direction] = (4 * W,)
    for n in range(2, d + 1):
        if deep:                        # every layer bidirectional, 2W-wide inputs (seq2seq.py:273-276)
            for direction in ('fw', 'bw'):
                shapes['enc%d_%s_K' % (n, direction)] = (2 * W, 4 * W)
                shapes['enc%d_%s_R' % (n, direction)] = (W, 4 * W)
                shapes['enc%d_%s_b' % (n, direction)] = (4 * W,)
            continue
        shapes['enc%d_K' % n] = (2 * W if n == 2 else W, 4 * W)
        shapes['enc%d_R' % n] = (W, 4 * W)
        shapes['enc%d_b' % n] = (4 * W,)
    shapes['att_U'] = (C, W)
    for n in range(1, d):
        shapes['dec%d_K' % n] = (W, 4 * W)
        shapes['dec%d_R' % n] = (W, 4 * W)
        shapes['dec%d_b' % n] = (4 * W,)
    shapes['att_Wa'] = (W, W)
    shapes['att_va'] = (W,)
    shapes['att_bUW'] = (W,)
    shapes['att_bv'] = (1,)
    shapes['dec%d_K' % d] = (W + C, 4 * W)
    shapes['dec%d_R' % d] = (W, 4 * W)
    shapes['dec%d_b' % d] = (4 * W,)
    if bridge_dense:
        for n in range(1, d + 1):
            for part in ('h', 'c'):
                shapes['bridge%d_%s_K' % (n, part)] = (W, W)
                shapes['bridge%d_%s_b' % (n, part)] = (W,)
    return shapes


def _pad_blocks(a, axis, blocks, W, Wp):
    """Along `axis`, `a` consists of `blocks` consecutive blocks of W entries: widen every block to Wp with zeros."""
    if W == Wp:
        return a
    a = np.asarray(a)
    shape = list(a.shape)
    assert shape[axis] == blocks * W, (shape, axis, blocks, W)
    a = np.moveaxis(a, axis, -1).reshape(a.shape[:axis] + a.shape[axis + 1:] + (blocks, W))
    out = np.zeros(a.shape[:-1] + (Wp,), a.dtype)
    out[..., :W] = a
    out = out.reshape(out.shape[:-2] + (blocks * Wp,))
    return np.ascontiguousarray(np.moveaxis(out, -1, axis))


def _strip_blocks(a, axis, blocks, W, Wp):
    """Inverse of _pad_blocks."""
    if W == Wp:
        return a
    a = np.asarray(a)
    a = np.moveaxis(a, axis, -1)
    a = a.reshape(a.shape[:-1] + (blocks, Wp))[..., :W]
    a = a.reshape(a.shape[:-2] + (blocks * W,))
    return np.ascontiguousarray(np.moveaxis(a, -1, axis))


def _width_blocks(name, depth, deep=False):
    """(blocks along axis 0, blocks along axis 1 or None) of the hidden width in a Keras-layout tensor of weight_shapes()."""
    d = depth
    top = 'dec%d_' % d
    if name == 'E':
        return (None, 1)
    if name.startswith('bridge'):
        return (1, 1) if name.endswith('_K') else (1, None)
    if name in ('att_va', 'att_bUW'):
        return (1, None)
    if name == 'att_bv':
        return (None, None)
    if name == 'att_U':
        return (2 if (d == 1 or deep) else 1, 1)
    if name == 'att_Wa':
        return (1, 1)
    if name.endswith('_b'):
        return (4, None)
    if name.endswith('_R'):
        return (1, 4)
    if name.endswith('_K'):
        if name == 'enc2_K' or (deep and name.startswith('enc') and not name.startswith('enc1_')):
            return (2, 4)
        if name == top + 'K':
            return (3 if (d == 1 or deep) else 2, 4)       # input + context (2W wide at depth 1 / with a deep bidirectional encoder)
        return (1, 4)
    raise KeyError(name)


class HipEngine(object):
    """One model handle on one HIP device.

    Hidden widths that are not a multiple of 32 (the C ABI's tile granularity; the reference's `--width` takes any integer) are
    padded here with dead units: every tensor crosses the ABI widened to the next multiple of 32, block by block, with zeros.
    That is exact, not approximate: a unit whose incoming weights, outgoing weights and biases are all zero has gate
    pre-activations 0, hence c' = f*c + i*tanh(0) = 0 and h = o*tanh(0) = 0 at every step, feeds nothing into any real unit,
    reads nothing from one, has zero attention weight (v_a = 0) -- and receives exactly zero gradient, so Adam leaves it at zero."""

    def __init__(self, depth, width, voc_size, device=0, window_width=5, residual_connections=False,
                 deep_bidirectional_encoder=False, bridge_dense=False, lm=False, stateful=False):
        self.lib = nv.load()
        self.depth, self.width, self.voc_size = int(depth), int(width), int(voc_size)
        if self.width < 1:
            raise ValueError('width must be positive')
        self.pwidth = (self.width + 31) // 32 * 32            # what the device sees
        self.deep = bool(deep_bidirectional_encoder)
        if self.deep and self.width % 32:
            # (the "cross sum" of seq2seq.py:246-259 pairs neighbouring features of [fw | bw]: dead-unit padding would move the pairs)
            raise ValueError('deep_bidirectional_encoder needs a width that is a multiple of 32')
        self.ctx_width = 2 * self.width if (self.depth == 1 or self.deep) else self.width
        self.cblocks = 2 if (self.depth == 1 or self.deep) else 1
        self.window_width = int(window_width)
        cfg = nv.Config(self.depth, self.pwidth, self.voc_size, int(window_width), int(bool(residual_connections)),
                        int(bool(deep_bidirectional_encoder)), int(bool(bridge_dense)), int(bool(lm)),
                        int(bool(stateful)))
        handle = c_void_p()
        nv.check(self.lib.casv_model_create(byref(cfg), int(device), byref(handle)))
        self.handle = handle
        self.residual_connections, self.bridge_dense = bool(residual_connections), bool(bridge_dense)
        self.shapes = weight_shapes(self.depth, self.width, self.voc_size, self.bridge_dense, self.deep)
        self.pshapes = weight_shapes(self.depth, self.pwidth, self.voc_size, self.bridge_dense, self.deep)
        self.B = self.T = 0
        self._score_shape = None            # (rows, U) of this object's last scoring call (score_alternatives)

    # -- dead-unit padding (class docstring) ---------------------------------------------------
    def _pad_weight(self, name, a):
        W, Wp = self.width, self.pwidth
        if W == Wp:
            return a
        b0, b1 = _width_blocks(name, self.depth, self.deep)
        a = np.asarray(a, np.float32).reshape(self.shapes[name])
        if b0:
            a = _pad_blocks(a, 0, b0, W, Wp)
        if b1:
            a = _pad_blocks(a, 1, b1, W, Wp)
        return a

    def _strip_weight(self, name, a):
        W, Wp = self.width, self.pwidth
        if W == Wp:
            return a
        b0, b1 = _width_blocks(name, self.depth, self.deep)
        a = np.asarray(a).reshape(self.pshapes[name])
        if b0:
            a = _strip_blocks(a, 0, b0, W, Wp)
        if b1:
            a = _strip_blocks(a, 1, b1, W, Wp)
        return a

    def _padw(self, a, blocks=1):
        """Widen the LAST axis (blocks x width) of a state / output array."""
        return _pad_blocks(np.asarray(a, np.float32), np.asarray(a).ndim - 1, blocks, self.width, self.pwidth)

    def _stripw(self, a, blocks=1):
        return _strip_blocks(a, np.asarray(a).ndim - 1, blocks, self.width, self.pwidth)

    def close(self):
        if getattr(self, 'handle', None):
            self.lib.casv_model_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- weights -------------------------------------------------------------------------------
    def set_weights(self, weights):
        for name, shape in self.shapes.items():
            if name not in weights:
                raise KeyError('missing weight "%s"' % name)
            a = nv.carray(weights[name], np.float32)
            if tuple(a.shape) != tuple(shape) and a.size != int(np.prod(shape)):
                raise ValueError('weight "%s" has shape %s, expected %s' % (name, a.shape, shape))
            a = nv.carray(self._pad_weight(name, a), np.float32)
            nv.check(self.lib.casv_set_weight(self.handle, name.encode(), nv.ptr(a), a.size))
        nv.check(self.lib.casv_commit_weights(self.handle))

    def get_weights(self):
        out = {}
        for name, shape in self.pshapes.items():
            a = np.empty(shape, np.float32)
            nv.check(self.lib.casv_get_weight(self.handle, name.encode(), nv.ptr(a), a.size))
            out[name] = self._strip_weight(name, a)
        return out

    # -- encoder -------------------------------------------------------------------------------
    @staticmethod
    def source_rejection(idx, val):
        """The rejection candidate of every input position: argmax of its input row, -1 for all-zero rows (seq2seq.py:1458-1462).
        idx / val (B,T,A).  (Host arithmetic on the whole batch: callers that prepare batches ahead of the device stage compute
        it there and hand it to encode().)"""
        masked = np.where(idx >= 0, val, -np.inf)
        best = masked.max(axis=2, keepdims=True)
        cand = np.where((masked == best) & (idx >= 0), idx, np.iinfo(np.int32).max)
        src_rej = cand.min(axis=2)
        anyval = ((idx >= 0) & (val != 0)).any(axis=2)
        return np.where(anyval, src_rej, -1).astype(np.int32)

    def encode(self, idx, val=None, src_rej=None):
        """idx int32 (B,T) or (B,T,A) with -1 for empty slots; val float32 same shape (default 1)."""
        idx = nv.carray(idx, np.int32)
        if idx.ndim == 2:
            idx = idx[:, :, None]
        idx = np.ascontiguousarray(idx)
        B, T, A = idx.shape
        if val is None:
            val = np.ones(idx.shape, np.float32)
        val = nv.carray(np.broadcast_to(np.asarray(val, np.float32).reshape(B, T, -1), idx.shape), np.float32)
        if src_rej is None:
            src_rej = self.source_rejection(idx, val)
        src_rej = nv.carray(src_rej, np.int32)
        nv.check(self.lib.casv_encode(self.handle, B, T, A, nv.ptr(idx), nv.ptr(val), nv.ptr(src_rej)))
        self.B, self.T = B, T

    def set_encoder_outputs(self, enc_out, states, a0=None, src_rej=None):
        """Install encoder outputs computed elsewhere: enc_out (B,T,C), states [h1,c1,...,hd,cd] each (B,W), a0 (B,T) or None."""
        enc_out = nv.carray(self._padw(enc_out, self.cblocks), np.float32)
        B, T = enc_out.shape[:2]
        st = nv.carray(self._padw(np.stack([np.asarray(x, np.float32).reshape(B, self.width) for x in states[:2 * self.depth]])), np.float32)
        a0 = None if a0 is None else nv.carray(np.asarray(a0, np.float32).reshape(B, T), np.float32)
        src_rej = None if src_rej is None else nv.carray(src_rej, np.int32)
        nv.check(self.lib.casv_set_encoder_outputs(self.handle, B, T, nv.ptr(enc_out), nv.ptr(st), nv.ptr(a0), nv.ptr(src_rej)))
        self.B, self.T = B, T

    def encoder_outputs(self):
        enc = np.empty((self.B, self.T, self.cblocks * self.pwidth), np.float32)
        st = np.empty((2 * self.depth, self.B, self.pwidth), np.float32)
        nv.check(self.lib.casv_get_encoder_outputs(self.handle, nv.ptr(enc), nv.ptr(st)))
        enc, st = self._stripw(enc, self.cblocks), self._stripw(st)
        return enc, [st[i] for i in range(2 * self.depth)]

    def debug_u(self):
        """Test support (casv_debug_get_u): u = attention_dense(enc_out) of the last encoder pass, (B, T, padded width) as on the device."""
        u = np.empty((self.B, self.T, self.pwidth), np.float32)
        nv.check(self.lib.casv_debug_get_u(self.handle, nv.ptr(u)))
        return u

    def decoder_step(self, line, p_in, states, a_in):
        line = nv.carray(line, np.int32)
        R = line.shape[0]
        p_in = nv.carray(p_in, np.float32)
        st = nv.carray(self._padw(np.stack(states[:2 * self.depth])), np.float32)
        a_in = nv.carray(a_in, np.float32)
        probs = np.empty((R, self.voc_size), np.float32)
        st_out = np.empty_like(st)
        a_out = np.empty((R, self.T), np.float32)
        nv.check(self.lib.casv_decoder_step(self.handle, R, nv.ptr(line), nv.ptr(p_in), nv.ptr(st), nv.ptr(a_in),
                                            nv.ptr(probs), nv.ptr(st_out), nv.ptr(a_out)))
        st_out = self._stripw(st_out)
        return probs, [st_out[i] for i in range(2 * self.depth)] + [a_out]

    def decoder_step_lm(self, line, p_in, states, a_in):
        """decoder_step plus the LM output of lm_predict (casv_decoder_step_lm): (probs, lm_probs, new states)."""
        line = nv.carray(line, np.int32)
        R = line.shape[0]
        p_in = nv.carray(p_in, np.float32)
        st = nv.carray(self._padw(np.stack(states[:2 * self.depth])), np.float32)
        a_in = nv.carray(a_in, np.float32)
        probs = np.empty((R, self.voc_size), np.float32)
        lm_probs = np.empty((R, self.voc_size), np.float32)
        st_out = np.empty_like(st)
        a_out = np.empty((R, self.T), np.float32)
        nv.check(self.lib.casv_decoder_step_lm(self.handle, R, nv.ptr(line), nv.ptr(p_in), nv.ptr(st), nv.ptr(a_in),
                                               nv.ptr(probs), nv.ptr(st_out), nv.ptr(a_out), nv.ptr(lm_probs)))
        st_out = self._stripw(st_out)
        return probs, lm_probs, [st_out[i] for i in range(2 * self.depth)] + [a_out]

    # -- decode loops --------------------------------------------------------------------------
    def decode_greedy(self, mode=0, steps=None, want_align=False):
        S = int(steps or 2 * self.T)
        idx = np.empty((self.B, S), np.int32)
        prob = np.empty((self.B, S), np.float32)
        length = np.empty((self.B,), np.int32)
        sparse = want_align == 'sparse'        # (lo, w) windows instead of (B, S, T) rows
        align = np.empty((self.B, S, self.T), np.float32) if want_align and not sparse else None
        nv.check(self.lib.casv_decode_greedy(self.handle, int(mode), S, nv.ptr(idx), nv.ptr(prob), nv.ptr(length),
                                             nv.ptr(align)))
        if sparse:
            align = self.alignments_sparse(self.B, S)
        return idx, prob, length, align

    def decode_beam(self, batch_size=8, beam_width_in=15, beam_threshold_in=0.2, beam_width_out=16,
                    rejection_threshold=0.3, cost0=3.0, max_results=1, steps=None, want_align=False):
        S = int(steps or 2 * self.T)
        MR = int(max_results)
        p = nv.BeamParams(int(batch_size), int(beam_width_in), int(beam_width_out), MR, float(beam_threshold_in),
                          float(rejection_threshold or 0.0), float(cost0))
        n = self.B * MR
        out = {'idx': np.empty((n, S), np.int32), 'prob': np.empty((n, S), np.float32),
               'len': np.empty((n,), np.int32), 'score': np.empty((n,), np.float64),
               'rej': np.empty((n, S), np.int32),
               'align': np.empty((n, S, self.T), np.float32) if want_align and want_align != 'sparse' else None,
               'n_found': np.empty((self.B,), np.int32), 'n_steps': np.empty((self.B,), np.int32)}
        nv.check(self.lib.casv_decode_beam(self.handle, byref(p), S, nv.ptr(out['idx']), nv.ptr(out['prob']),
                                           nv.ptr(out['len']), nv.ptr(out['score']), nv.ptr(out['rej']),
                                           nv.ptr(out['align']), nv.ptr(out['n_found']), nv.ptr(out['n_steps'])))
        if want_align == 'sparse':
            out['align_sparse'] = self.alignments_sparse(n, S)
        return out

    def decode_sample(self, samples, temperature=1.0, top_k=0, seed=0, streams=None, steps=None, want_align=False):
        return self._decode_sample(None, samples, temperature, top_k, seed, streams, steps, want_align)

    def decode_sample_cut(self, samples, temperature=1.0, top_k=0, top_p=1.0, seed=0, streams=None, steps=None, want_align=False):
        """casv_decode_sample_cut: decode_sample under the cut (top_k in 0 .. 4095, top_p in (0, 1]; DESIGN.md section 4.8, items 11
        to 13): every draw comes from the first top_k candidates in rank order, and of those from the nucleus whose float64 mass
        first reaches top_p.  Returns what decode_sample returns."""
        return self._decode_sample(nv.SampleCut(int(top_k), float(top_p)), samples, temperature, 0, seed, streams, steps, want_align)

    def _decode_sample(self, cut, samples, temperature, top_k, seed, streams, steps, want_align):
        """casv_decode_sample: `samples` lines drawn from the decoder for every encoded line.  Returns
        (idx, logp, logq (B, samples, S), length (B, samples), align): the drawn indices, their log-probabilities under the model and
        under the proposal, the steps up to and including the first end-of-line, and (B, samples, S, T) alignment rows, their
        (lo, w) windows with want_align='sparse', or None.  streams (B) int64: the lines' stream ids (default: their numbers).
        An invalid row raises NativeError (CASV_ERR_NAN) whose `outputs` holds the same tuple, filled."""
        S = int(steps or 2 * self.T)
        N = int(samples)
        rows = self.B * max(N, 0)
        p = nv.SampleParams(int(seed) & 0xFFFFFFFFFFFFFFFF, float(temperature), int(top_k), N)
        if streams is not None:
            streams = nv.carray(streams, np.int64)
            assert streams.shape == (self.B,)
        idx = np.empty((rows, S), np.int32)
        logp = np.empty((rows, S), np.float32)
        logq = np.empty((rows, S), np.float32)
        length = np.empty((rows,), np.int32)
        sparse = want_align == 'sparse'
        align = np.empty((rows, S, self.T), np.float32) if want_align and not sparse else None
        if cut is None:
            rc = self.lib.casv_decode_sample(self.handle, byref(p), S, nv.ptr(streams), nv.ptr(idx), nv.ptr(logp), nv.ptr(logq),
                                             nv.ptr(length), nv.ptr(align))
        else:
            rc = self.lib.casv_decode_sample_cut(self.handle, byref(p), byref(cut), S, nv.ptr(streams), nv.ptr(idx), nv.ptr(logp),
                                                 nv.ptr(logq), nv.ptr(length), nv.ptr(align))
        if rc not in (0, nv.CASV_ERR_NAN):
            nv.check(rc)
        if sparse:
            lo, w = self.alignments_sparse(rows, S)
            align = (lo.reshape(self.B, N, S), w.reshape(self.B, N, S, -1))
        elif align is not None:
            align = align.reshape(self.B, N, S, self.T)
        out = (idx.reshape(self.B, N, S), logp.reshape(self.B, N, S), logq.reshape(self.B, N, S), length.reshape(self.B, N), align)
        if rc:
            err = nv.NativeError(rc, self.lib.casv_last_error().decode('utf-8', 'replace'))
            err.outputs = out
            raise err
        return out

    def debug_sample_rows(self, logits, temperature=1.0, top_k=0, seed=0, step=0, streams=None, samples=None, u=None, pad_value=0.0):
        return self._debug_sample_rows(None, logits, temperature, top_k, seed, step, streams, samples, u, pad_value)

    def debug_sample_cut_rows(self, logits, temperature=1.0, top_k=0, top_p=1.0, seed=0, step=0, streams=None, samples=None, u=None,
                              pad_value=0.0):
        """Test support (casv_debug_sample_cut_rows): debug_sample_rows under the cut (top_k, top_p), by sample_cut_kernel;
        stat('sample_cut_rows') then tells the rows per workgroup of the launch."""
        return self._debug_sample_rows(nv.SampleCut(int(top_k), float(top_p)), logits, temperature, 0, seed, step, streams, samples, u,
                                       pad_value)

    def _debug_sample_rows(self, cut, logits, temperature, top_k, seed, step, streams, samples, u, pad_value):
        """Test support (casv_debug_sample_rows): the sampling kernel alone on logits (R,V) as step `step` of rows with stream ids
        streams (R; default: the row's number) and sample numbers samples (R; default 0); u (R): these uniforms instead of the
        generator's; the padding columns of the device rows hold pad_value.  Returns (idx, logp, logq (R), feedback (R,Vp))."""
        logits = nv.carray(logits, np.float32)
        R, V = logits.shape
        p = nv.SampleParams(int(seed) & 0xFFFFFFFFFFFFFFFF, float(temperature), int(top_k), 1)
        streams = None if streams is None else nv.carray(streams, np.int64)
        samples = None if samples is None else nv.carray(samples, np.int32)
        u = None if u is None else nv.carray(u, np.float32)
        for a in (streams, samples, u):
            assert a is None or a.shape == (R,)
        idx = np.empty((R,), np.int32)
        logp = np.empty((R,), np.float32)
        logq = np.empty((R,), np.float32)
        feedback = np.empty((R, (V + 31) & ~31), np.float32)
        if cut is None:
            nv.check(self.lib.casv_debug_sample_rows(self.handle, R, V, byref(p), int(step), nv.ptr(streams), nv.ptr(samples), nv.ptr(logits),
                                                     nv.ptr(u), float(pad_value), nv.ptr(idx), nv.ptr(logp), nv.ptr(logq), nv.ptr(feedback)))
        else:
            nv.check(self.lib.casv_debug_sample_cut_rows(self.handle, R, V, byref(p), byref(cut), int(step), nv.ptr(streams), nv.ptr(samples),
                                                         nv.ptr(logits), nv.ptr(u), float(pad_value), nv.ptr(idx), nv.ptr(logp), nv.ptr(logq),
                                                         nv.ptr(feedback)))
        return idx, logp, logq, feedback

    # -- training ------------------------------------------------------------------------------
    def train_begin(self, lr=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-7, clipnorm=5.0, frozen=()):
        p = nv.AdamParams(lr, beta1, beta2, epsilon, clipnorm)
        csv = ','.join(frozen).encode() if frozen else None
        self._frozen = tuple(frozen)
        nv.check(self.lib.casv_train_begin(self.handle, byref(p), csv))

    def _step_masks(self, masks):
        """The train step's three mask arrays (enc, dec, cell) in the device's padded widths, or None each without masks."""
        if masks is None:
            return None, None, None
        # (dead units are multiplied by zero whatever their mask says)
        m_enc = nv.carray(np.concatenate([self._padw(np.asarray(x, np.float32).ravel(), 2 if (n == 0 or self.deep) else 1)
                                          for n, x in enumerate(masks['enc'])]), np.float32)
        m_dec = None
        if self.depth > 1:
            m_dec = nv.carray(np.concatenate([self._padw(np.asarray(x, np.float32).ravel()) for x in masks['dec']]), np.float32)
        m_cell = nv.carray(self._padw(np.asarray(masks['cell'], np.float32), 1 + self.cblocks), np.float32)
        return m_enc, m_dec, m_cell

    @staticmethod
    def _encoder_batch(enc_idx, enc_val):
        """The encoder's half of a batch as the library takes it: enc_idx (B,T,A) int32 (from (B,T[,A])), enc_val float32 of that
        shape or None, and (B, T, A)."""
        enc_idx = nv.carray(enc_idx, np.int32)
        if enc_idx.ndim == 2:
            enc_idx = np.ascontiguousarray(enc_idx[:, :, None])
        B, T, A = enc_idx.shape
        enc_val = None if enc_val is None else nv.carray(np.asarray(enc_val, np.float32).reshape(B, T, A), np.float32)
        return enc_idx, enc_val, (B, T, A)

    def _step_batch(self, enc_idx, enc_val, dec_in):
        """_encoder_batch and the decoder input (B,U) int32 beside it: enc_idx, enc_val, dec_in, (B, T, A, U)."""
        enc_idx, enc_val, (B, T, A) = self._encoder_batch(enc_idx, enc_val)
        dec_in = nv.carray(dec_in, np.int32)
        return enc_idx, enc_val, dec_in, (B, T, A, dec_in.shape[1])

    def _step_call(self, entry, mode, batch, targets, weights, masks, extra=()):
        """One call of a casv_train_step* entry on a _step_batch: the common arguments with the entry's targets between dec_in and
        the weights and what else it takes (`extra`) in front of loss and norm.  Returns (loss, grad_norm)."""
        enc_idx, enc_val, dec_in, (B, T, A, U) = batch
        loss, norm = c_double(), c_double()
        nv.check(entry(self.handle, int(mode), B, T, U, A, nv.ptr(enc_idx), nv.ptr(enc_val), nv.ptr(dec_in), *targets, nv.ptr(weights),
                       *[nv.ptr(m) for m in self._step_masks(masks)], *extra, byref(loss), byref(norm)))
        return loss.value, norm.value

    def train_step(self, enc_idx, enc_val, dec_in, dec_out, weights, masks=None, mode=1):
        """One train_on_batch (mode 1), test_on_batch (mode 0) or loss+gradients (mode 2).
        enc_idx (B,T[,A]) int32, dec_in/dec_out (B,U) int32 (-1 = zero row), weights (B,U).
        masks: {'enc': [..], 'dec': [..], 'cell': (B,W+C)} of scaled keep-masks, or None."""
        batch = self._step_batch(enc_idx, enc_val, dec_in)
        dec_out = nv.carray(dec_out, np.int32)
        return self._step_call(self.lib.casv_train_step, mode, batch, (nv.ptr(dec_out),), nv.carray(weights, np.float32), masks)

    def train_step_soft(self, enc_idx, enc_val, dec_in, soft_idx, soft_q, weights, masks=None, mode=1):
        """train_step on soft targets (casv_train_step_soft): soft_idx int32 / soft_q float32 (B,U,K) hold K (index, mass) slots
        per position in place of dec_out -- index -1 = empty slot, all empty = zero row, masses finite and >= 0, a position's indices
        distinct, 1 <= K <= min(V, 64) (NativeError CASV_ERR_ARG otherwise, nothing touched).  One slot (dec_out, 1.0) is the hard
        step.  Everything else as train_step; returns (loss, grad_norm)."""
        batch = self._step_batch(enc_idx, enc_val, dec_in)
        (B, _, _, U) = batch[3]
        soft_idx = nv.carray(soft_idx, np.int32)
        soft_q = nv.carray(soft_q, np.float32)
        weights = nv.carray(weights, np.float32)
        assert soft_idx.ndim == 3 and soft_idx.shape[:2] == (B, U) and soft_q.shape == soft_idx.shape and weights.shape == (B, U)
        return self._step_call(self.lib.casv_train_step_soft, mode, batch, (soft_idx.shape[2], nv.ptr(soft_idx), nv.ptr(soft_q)), weights, masks)

    def train_step_risk(self, enc_idx, enc_val, dec_in, dec_out, weights, cost, n, alpha=1.0, masks=None, mode=1, details=False):
        """train_step with the minimum-risk head (casv_train_step_risk): the B rows are B // n groups of n candidate lines, row
        g * n + i = candidate i of group g; cost (B) float32, a finite value >= 0 = a member with that cost, negative = not a
        member.  The loss is the mean over the groups with a member of sum_i q_i cost_i, q the model's distribution renormalised
        over the group's members with sharpness alpha.  mode 1 or 2; 1 <= n <= 64, B a multiple of n, costs finite, alpha finite and
        > 0 (NativeError CASV_ERR_ARG otherwise, nothing touched).  Returns (loss, grad_norm), with details=True (loss, grad_norm,
        q (B) float64, risk (B // n) float64)."""
        batch = self._step_batch(enc_idx, enc_val, dec_in)
        (B, _, _, U) = batch[3]
        dec_out = nv.carray(dec_out, np.int32)
        weights = nv.carray(weights, np.float32)
        cost = None if cost is None else nv.carray(cost, np.float32)
        assert dec_out.shape == (B, U) and weights.shape == (B, U) and (cost is None or cost.shape == (B,))
        n = int(n)
        q = np.empty((B,), np.float64) if details else None
        risk = np.empty((max(B // max(n, 1), 1),), np.float64) if details else None
        out = self._step_call(self.lib.casv_train_step_risk, mode, batch, (nv.ptr(dec_out),), weights, masks,
                              (n, nv.ptr(cost), float(alpha), nv.ptr(q), nv.ptr(risk)))
        return out + (q, risk[:B // n]) if details else out

    @staticmethod
    def _sched_params(seed, step_id, ratio, pick, passes, temperature):
        picks = {'greedy': 0, 'sample': 1}
        return nv.SchedParams(int(seed) & 0xFFFFFFFFFFFFFFFF, int(step_id) & 0xFFFFFFFFFFFFFFFF, float(ratio), float(temperature),
                              picks.get(pick, pick), int(passes))

    def train_step_sampled(self, enc_idx, enc_val, dec_in, dec_out, weights, masks=None, mode=1, ratio=0.0, seed=0, step_id=0,
                           pick='greedy', passes=1, temperature=1.0, top_k=0, top_p=1.0):
        """train_step with scheduled sampling in its parallel form (casv_train_step_sampled): after the teacher-forced forward
        pass, `passes` times a pick ('greedy' or 'sample' at `temperature`) at every decoder position from the logits of the
        position before it, mixed into the decoder input where the position's coin -- a function of (seed, step_id, b, u) -- falls
        below `ratio`, and the decoder again; loss, backward pass and update on the last pass.  Modes 1 and 2 only.  Returns
        (loss, grad_norm, mixes) with mixes int32 (passes,B,U): slice p - 1 is the decoder input after pass p.  top_k / top_p:
        the 'sample' pick draws under this cut (casv_train_step_sampled_cut, called only when one of them is set)."""
        batch = self._step_batch(enc_idx, enc_val, dec_in)
        (B, _, _, U) = batch[3]
        dec_out = nv.carray(dec_out, np.int32)
        p = self._sched_params(seed, step_id, ratio, pick, passes, temperature)
        mixes = np.empty((max(int(passes), 0), B, U), np.int32)
        entry, extra = self.lib.casv_train_step_sampled, (byref(p), nv.ptr(mixes))
        if not (top_k == 0 and top_p == 1.0):
            cut = nv.SampleCut(int(top_k), float(top_p))
            entry, extra = self.lib.casv_train_step_sampled_cut, (byref(p), byref(cut), nv.ptr(mixes))
        return self._step_call(entry, mode, batch, (nv.ptr(dec_out),), nv.carray(weights, np.float32), masks, extra) + (mixes,)

    def debug_sched_rows(self, logits, gold, b, u, ratio=1.0, seed=0, step_id=0, pick='greedy', temperature=1.0, pad_value=0.0):
        """Test support (casv_debug_sched_rows): the mix kernel alone on logits (R,V) -- row r is decoder position (b[r], u[r])
        with the gold input gold[r]; the padding columns of the device rows hold pad_value.  Returns the mix (R) int32."""
        return self._debug_sched_rows(None, logits, gold, b, u, ratio, seed, step_id, pick, temperature, pad_value)

    def debug_sched_cut_rows(self, logits, gold, b, u, ratio=1.0, seed=0, step_id=0, pick='sample', temperature=1.0, top_k=0, top_p=1.0,
                             pad_value=0.0):
        """Test support (casv_debug_sched_cut_rows): debug_sched_rows with the sampled pick under the cut (top_k, top_p)."""
        return self._debug_sched_rows(nv.SampleCut(int(top_k), float(top_p)), logits, gold, b, u, ratio, seed, step_id, pick, temperature,
                                      pad_value)

    def _debug_sched_rows(self, cut, logits, gold, b, u, ratio, seed, step_id, pick, temperature, pad_value):
        logits = nv.carray(logits, np.float32)
        R, V = logits.shape
        gold, b, u = (nv.carray(a, np.int32) for a in (gold, b, u))
        assert gold.shape == b.shape == u.shape == (R,)
        p = self._sched_params(seed, step_id, ratio, pick, 1, temperature)
        out = np.empty((R,), np.int32)
        rows = (nv.ptr(b), nv.ptr(u), nv.ptr(logits), nv.ptr(gold), float(pad_value), nv.ptr(out))
        if cut is None:
            nv.check(self.lib.casv_debug_sched_rows(self.handle, R, V, byref(p), *rows))
        else:
            nv.check(self.lib.casv_debug_sched_cut_rows(self.handle, R, V, byref(p), byref(cut), *rows))
        return out

    def train_gradients(self):
        out = {}
        for name, shape in self.pshapes.items():
            a = np.empty(shape, np.float32)
            nv.check(self.lib.casv_train_get_gradient(self.handle, name.encode(), nv.ptr(a), a.size))
            out[name] = self._strip_weight(name, a)
        return out

    def train_state(self):
        """Adam's state of the session in Keras layout: ({name: m}, {name: v}, step); frozen tensors have none."""
        ms, vs = {}, {}
        frozen = tuple(getattr(self, '_frozen', ()))
        for name, shape in self.pshapes.items():
            if any(name.startswith(p) for p in frozen):
                continue
            for which, out in ((0, ms), (1, vs)):
                a = np.empty(shape, np.float32)
                nv.check(self.lib.casv_train_get_state(self.handle, name.encode(), which, nv.ptr(a), a.size))
                out[name] = self._strip_weight(name, a)
        step = c_int64()
        nv.check(self.lib.casv_train_get_step(self.handle, byref(step)))
        return ms, vs, step.value

    def set_train_state(self, m, v, step):
        """Set Adam's moments ({name: array} in Keras layout, as train_state returns them) and step count into the session."""
        for which, src in ((0, m), (1, v)):
            for name, a in src.items():
                a = nv.carray(self._pad_weight(name, nv.carray(a, np.float32)), np.float32)
                nv.check(self.lib.casv_train_set_state(self.handle, name.encode(), which, nv.ptr(a), a.size))
        nv.check(self.lib.casv_train_set_step(self.handle, int(step)))

    def train_weights(self):
        nv.check(self.lib.casv_train_sync_weights(self.handle))
        return self.get_weights()

    def train_end(self):
        nv.check(self.lib.casv_train_end(self.handle))

    # -- scoring -------------------------------------------------------------------------------
    def _score_call(self, entry, rows, U, T, head, want_align):
        """One scoring call: `head` = the entry's arguments up to dec_out, rows = (B,) or (B, N).  Returns (logp, best, rank
        rows + (U,), nll, count rows, align) with the alignments as want_align asks: None, dense rows + (U, T), or ('sparse') the
        window form (lo rows + (U,), w rows + (U, K)) of casv_score_get_alignments_sparse."""
        logp, best, rank = np.empty(rows + (U,), np.float32), np.empty(rows + (U,), np.int32), np.empty(rows + (U,), np.int32)
        nll, count = np.empty(rows, np.float64), np.empty(rows, np.int32)
        sparse = want_align == 'sparse'
        align = np.empty(rows + (U, T), np.float32) if want_align and not sparse else None
        nv.check(entry(self.handle, *head, nv.ptr(logp), nv.ptr(best), nv.ptr(rank), nv.ptr(nll), nv.ptr(count), nv.ptr(align)))
        self._score_shape = (int(np.prod(rows)), U)          # (score_alternatives: the rows the library now holds)
        if sparse:
            K = 2 * self.window_width + 1
            align = (np.empty(rows + (U,), np.int32), np.empty(rows + (U, K), np.float32))
            nv.check(self.lib.casv_score_get_alignments_sparse(self.handle, K, nv.ptr(align[0]), nv.ptr(align[1])))
        return logp, best, rank, nll, count, align

    def score_targets(self, enc_idx, enc_val, dec_in, dec_out, want_align=False):
        """Teacher-forced log-probabilities of the targets dec_out (casv_score_targets; arrays as train_step, no weights, no masks).
        Returns (logp float32 (B,U), best int32 (B,U), rank int32 (B,U), nll float64 (B), count int32 (B), align) with align = None,
        the dense rows (B,U,T) (want_align=True) or the window form (lo (B,U), w (B,U,K)) (want_align='sparse').  Inside a training
        session the session's weights score, outside one the committed weights (a forward-only state kept until score_release)."""
        enc_idx, enc_val, dec_in, (B, T, A, U) = self._step_batch(enc_idx, enc_val, dec_in)
        dec_out = nv.carray(dec_out, np.int32)
        assert dec_in.shape == dec_out.shape == (B, U)
        head = (B, T, U, A, nv.ptr(enc_idx), nv.ptr(enc_val), nv.ptr(dec_in), nv.ptr(dec_out))
        return self._score_call(self.lib.casv_score_targets, (B,), U, T, head, want_align)

    def score_candidates(self, enc_idx, enc_val, dec_in, dec_out, want_align=False):
        """N candidate targets per source on one encoder pass (casv_score_candidates): enc_idx / enc_val (B,T[,A]) as score_targets,
        dec_in / dec_out (B,N,U); candidate n of source b is decoder row b * N + n and reads source b's encoder pass.  A candidate
        whose dec_out row is all -1 is padding (a source with fewer than N candidates): logp 0, rank -1, count 0, nll 0.0.  Returns
        (logp (B,N,U), best (B,N,U), rank (B,N,U), nll float64 (B,N), count (B,N), align) with align = None, the dense rows (B,N,U,T)
        (want_align=True) or the window form (lo (B,N,U), w (B,N,U,K)) (want_align='sparse'); everything else as score_targets, whose
        results are this call's at N = 1."""
        enc_idx, enc_val, (B, T, A) = self._encoder_batch(enc_idx, enc_val)
        dec_in = nv.carray(dec_in, np.int32)
        dec_out = nv.carray(dec_out, np.int32)
        assert dec_in.ndim == 3 and dec_in.shape == dec_out.shape and dec_in.shape[0] == B
        N, U = dec_in.shape[1:]
        head = (B, N, T, U, A, nv.ptr(enc_idx), nv.ptr(enc_val), nv.ptr(dec_in), nv.ptr(dec_out))
        return self._score_call(self.lib.casv_score_candidates, (B, N), U, T, head, want_align)

    def score_alternatives(self, K, want_entropy=True):
        """The K likeliest characters and the entropy of every position of the LAST score_targets / score_candidates call
        (casv_score_get_alternatives), unscored positions included.  Returns (alt_idx int32 (rows,U,K), alt_logp float32 (rows,U,K),
        entropy float32 (rows,U) or None), rows = B, or B*N after score_candidates (row b * N + n); most probable first, ties to the
        lower index, alt_logp the bits score_targets returns for that index as target; -1 / NaN / NaN on an invalid row.  May be
        repeated with another K; NativeError (CASV_ERR_STATE) without a scoring call to read, CASV_ERR_ARG for K outside
        [1, min(V, 64)]."""
        K = int(K)
        # the shape is that of this object's last scoring call; without one no buffer is handed over, and the library -- which
        # checks K, then its state, then the pointers -- gives the error
        shape = self._score_shape
        alt_idx = alt_logp = entropy = None
        if shape is not None:
            width = min(max(K, 1), 64)      # (a K out of range is refused before anything is written)
            alt_idx = np.empty(shape + (width,), np.int32)
            alt_logp = np.empty(shape + (width,), np.float32)
            entropy = np.empty(shape, np.float32) if want_entropy else None
        nv.check(self.lib.casv_score_get_alternatives(self.handle, K, nv.ptr(alt_idx), nv.ptr(alt_logp), nv.ptr(entropy)))
        return alt_idx, alt_logp, entropy

    def score_release(self):
        """Drop the forward-only state score_targets keeps outside a training session (allowed when there is none)."""
        nv.check(self.lib.casv_score_release(self.handle))

    @staticmethod
    def _edit_costs(sym, key, costs):
        """(key int32 like sym or None, nv.EditCosts) of a costed call: costs is an `edit_costs.EditCosts` or (gap, sub, near, unit)."""
        if key is not None:
            key = nv.carray(key, np.int32)
            assert key.shape == sym.shape
        return key, nv.EditCosts(*(costs.as_tuple() if hasattr(costs, 'as_tuple') else costs))

    def consensus(self, sym, length, weights=None, mode=0, want_dist=False, key=None, costs=None):
        """The vote over N candidates per source (casv_consensus): sym (B,N,L) int32 symbols compared for equality only, length
        (B,N) in -1 .. L (-1: a padding candidate), weights (B,N) float64, not negative and finite, or None (all 1.0); mode 0 sums
        weight * distance, mode 1 weight * distance / max(the two lengths, 1).  Returns (risk float64 (B,N), pick int32 (B), dist
        int32 (B,N,N) or None): the unit-cost Levenshtein distances, each candidate's risk summed over the live candidates in
        ascending order (+inf for padding), and the live candidate of smallest risk, the lowest index among equals (-1: none).
        Needs no weights and no encoded batch, and changes nothing another call reads.  costs: None, or an
        `edit_costs.EditCosts` or (gap, sub, near, unit) -- then casv_consensus_costed: the distances are those under the costs,
        key (B,N,L) int32 or None names the characters that are near each other, mode 1 divides by unit x the longer length as
        well, and L is at most 2048."""
        assert costs is not None or key is None
        sym = nv.carray(sym, np.int32)
        length = nv.carray(length, np.int32)
        assert sym.ndim == 3 and length.shape == sym.shape[:2]
        B, N, L = sym.shape
        if weights is not None:
            weights = nv.carray(weights, np.float64)
            assert weights.shape == (B, N)
        risk = np.empty((B, N), np.float64)
        pick = np.empty((B,), np.int32)
        dist = np.empty((B, N, N), np.int32) if want_dist else None
        if costs is None:
            nv.check(self.lib.casv_consensus(self.handle, B, N, L, int(mode), nv.ptr(sym), nv.ptr(length), nv.ptr(weights), nv.ptr(dist),
                                             nv.ptr(risk), nv.ptr(pick)))
        else:
            key, c = self._edit_costs(sym, key, costs)
            nv.check(self.lib.casv_consensus_costed(self.handle, B, N, L, int(mode), nv.ptr(sym), nv.ptr(key), nv.ptr(length), nv.ptr(weights),
                                                    ctypes.byref(c), nv.ptr(dist), nv.ptr(risk), nv.ptr(pick)))
        return risk, pick, dist

    def consensus_align(self, sym, length, pivot, key=None, costs=None):
        """Every candidate of a source aligned to its pivot (casv_consensus_align): sym (B,N,L) int32 symbols, L at most 2048,
        length (B,N) in -1 .. L, pivot (B) the index of a live candidate or -1 to skip the source.  Returns (where int32 (B,N,L),
        ncol int32 (B)): per candidate symbol the pivot symbol it stands against (>= 0) or -1 - slot of its insertion, ALIGN_NONE
        beyond a length, and the columns of the source's confusion network.  The device keeps what `consensus_vote` reads.
        key, costs as in `consensus` -- then casv_consensus_align_costed: the path under the costs."""
        assert costs is not None or key is None
        sym = nv.carray(sym, np.int32)
        length = nv.carray(length, np.int32)
        pivot = nv.carray(pivot, np.int32)
        assert sym.ndim == 3 and length.shape == sym.shape[:2] and pivot.shape == sym.shape[:1]
        B, N, L = sym.shape
        where = np.empty((B, N, L), np.int32)
        ncol = np.empty((B,), np.int32)
        if costs is None:
            nv.check(self.lib.casv_consensus_align(self.handle, B, N, L, nv.ptr(sym), nv.ptr(length), nv.ptr(pivot), nv.ptr(where), nv.ptr(ncol)))
        else:
            key, c = self._edit_costs(sym, key, costs)
            nv.check(self.lib.casv_consensus_align_costed(self.handle, B, N, L, nv.ptr(sym), nv.ptr(key), nv.ptr(length), nv.ptr(pivot),
                                                          ctypes.byref(c), nv.ptr(where), nv.ptr(ncol)))
        self._align_shape = (B, N)
        return where, ncol

    def consensus_vote(self, C, weights=None):
        """The vote per column over what the last `consensus_align` left on the device (casv_consensus_vote): C columns per source,
        at least the largest ncol; weights (B,N) float64, not negative and finite, or None (all 1.0).  Returns (src int32 (B,C,N),
        mass float64 (B,C,N), best int32 (B,C)): the candidate position in the column (-1 a gap, -2 padding or no column), per
        class of equal entries at its lowest index the members' weights summed in ascending order (-1.0 elsewhere), and the
        representative of the largest mass, the lowest index among equals (-1: no column).  May be repeated with other weights."""
        shape = getattr(self, '_align_shape', None)
        if shape is None:
            nv.check(self.lib.casv_consensus_vote(self.handle, int(C), None, None, None, None))      # (answers CASV_ERR_STATE or _ARG)
        B, N = shape
        C = int(C)
        if weights is not None:
            weights = nv.carray(weights, np.float64)
            assert weights.shape == (B, N)
        src = np.empty((B, max(C, 0), N), np.int32)
        mass = np.empty((B, max(C, 0), N), np.float64)
        best = np.empty((B, max(C, 0)), np.int32)
        nv.check(self.lib.casv_consensus_vote(self.handle, C, nv.ptr(weights), nv.ptr(src), nv.ptr(mass), nv.ptr(best)))
        return src, mass, best

    def debug_set_align_budget(self, nbytes):
        """Test support (casv_debug_set_align_budget): the direction workspace of `consensus_align` in bytes, 0 = the default."""
        nv.check(self.lib.casv_debug_set_align_budget(self.handle, int(nbytes)))

    def debug_score_rows(self, logits, target, pad_value=0.0):
        """Test support (casv_debug_score_rows): the scoring head alone on logits (R,V) and targets (R); the padding columns of the
        device rows hold pad_value.  Returns (logp, best, rank)."""
        logits = nv.carray(logits, np.float32)
        target = nv.carray(target, np.int32)
        R, V = logits.shape
        assert target.shape == (R,)
        logp = np.empty((R,), np.float32)
        best = np.empty((R,), np.int32)
        rank = np.empty((R,), np.int32)
        nv.check(self.lib.casv_debug_score_rows(self.handle, R, V, nv.ptr(logits), nv.ptr(target), float(pad_value), nv.ptr(logp),
                                                nv.ptr(best), nv.ptr(rank)))
        return logp, best, rank

    def debug_alternatives_rows(self, logits, K, pad_value=0.0):
        """Test support (casv_debug_alternatives_rows): score_alternatives' kernel alone on logits (R,V); the padding columns of the
        device rows hold pad_value.  Returns (alt_idx (R,K), alt_logp (R,K), entropy (R))."""
        logits = nv.carray(logits, np.float32)
        R, V = logits.shape
        K = int(K)
        width = min(max(K, 1), 64)
        alt_idx = np.empty((R, width), np.int32)
        alt_logp = np.empty((R, width), np.float32)
        entropy = np.empty((R,), np.float32)
        nv.check(self.lib.casv_debug_alternatives_rows(self.handle, R, V, K, nv.ptr(logits), float(pad_value), nv.ptr(alt_idx),
                                                       nv.ptr(alt_logp), nv.ptr(entropy)))
        return alt_idx, alt_logp, entropy

    def debug_soft_ce_rows(self, logits, soft_idx, soft_q, weight, inv_count, pad_value=0.0, want_grad=True, ordered=False):
        """Test support (casv_debug_soft_ce_rows): the soft-target loss head alone on logits (R,V), slots soft_idx / soft_q (R,K) and
        weights (R); the padding columns of the device rows hold pad_value and are checked to come back as zeros.  Returns (loss
        float64, dlogits (R,V) or None)."""
        logits = nv.carray(logits, np.float32)
        soft_idx = nv.carray(soft_idx, np.int32)
        soft_q = nv.carray(soft_q, np.float32)
        weight = nv.carray(weight, np.float32)
        R, V = logits.shape
        assert soft_idx.ndim == 2 and soft_idx.shape[0] == R and soft_q.shape == soft_idx.shape and weight.shape == (R,)
        K = soft_idx.shape[1]
        loss = c_double()
        dlogits = np.empty((R, V), np.float32) if want_grad else None
        nv.check(self.lib.casv_debug_soft_ce_rows(self.handle, R, V, K, nv.ptr(logits), nv.ptr(soft_idx), nv.ptr(soft_q), nv.ptr(weight),
                                                  float(inv_count), float(pad_value), int(bool(want_grad)), byref(loss), nv.ptr(dlogits),
                                                  int(bool(ordered))))
        return loss.value, dlogits

    def debug_risk_rows(self, logits, target, weight, cost, n, alpha=1.0, pad_value=0.0, want_grad=True):
        """Test support (casv_debug_risk_rows): the minimum-risk head alone on logits (B,U,V), targets / weights (B,U) and cost (B),
        B = groups * n; the padding columns of the device rows hold pad_value and are checked to come back as zeros.  Returns
        (loss float64, q (B) float64, coef (B) float32, dlogits (B,U,V) or None)."""
        logits = nv.carray(logits, np.float32)
        target = nv.carray(target, np.int32)
        weight = nv.carray(weight, np.float32)
        cost = nv.carray(cost, np.float32)
        B, U, V = logits.shape
        n = int(n)
        assert target.shape == (B, U) and weight.shape == (B, U) and cost.shape == (B,) and n >= 1 and B % n == 0
        loss = c_double()
        q = np.empty((B,), np.float64)
        coef = np.empty((B,), np.float32)
        dlogits = np.empty((B, U, V), np.float32) if want_grad else None
        nv.check(self.lib.casv_debug_risk_rows(self.handle, B // n, n, U, V, nv.ptr(logits), nv.ptr(target), nv.ptr(weight), nv.ptr(cost),
                                               float(alpha), float(pad_value), int(bool(want_grad)), byref(loss), nv.ptr(q), nv.ptr(coef),
                                               nv.ptr(dlogits)))
        return loss.value, q, coef, dlogits

    # -- measurement ---------------------------------------------------------------------------
    def profile(self, enable=True):
        """0/False = off, 1/True = every kernel class, 2 = only the dominant kernel (fused LSTM GEMM)."""
        nv.check(self.lib.casv_profile(self.handle, int(enable)))

    def profile_read(self, name):
        launches, ms, fl, by = c_int64(), c_double(), c_double(), c_double()
        nv.check(self.lib.casv_profile_read(self.handle, name.encode(), byref(launches), byref(ms), byref(fl),
                                            byref(by)))
        return {'launches': launches.value, 'ms': ms.value, 'flops': fl.value, 'bytes': by.value}

    def set_option(self, key, value):
        nv.check(self.lib.casv_set_option(self.handle, key.encode(), int(value)))

    def debug_contract(self, A, Bt, bias=None, split_k=False, wave_groups=False, weight=False, k_major=False):
        """Test support (casv_debug_contract): C = A . Bt^T (+ bias) through the launcher all GEMMs of the path go through;
        k_major: A (K,M), Bt (K,N), C = A^T . Bt through the weight-gradient kernels."""
        A, Bt = nv.carray(A, np.float32), nv.carray(Bt, np.float32)
        if k_major:
            (K, M), N = A.shape, Bt.shape[1]
            assert Bt.shape[0] == K and bias is None
            C = np.empty((M, N), np.float32)
            nv.check(self.lib.casv_debug_contract(self.handle, 8, M, N, K, nv.ptr(A), nv.ptr(Bt), None, nv.ptr(C)))
            return C
        bias = None if bias is None else nv.carray(bias, np.float32)
        (M, K), N = A.shape, Bt.shape[0]
        assert Bt.shape[1] == K and (bias is None or bias.shape == (N,))
        C = np.empty((M, N), np.float32)
        flags = (1 if split_k else 0) | (2 if wave_groups else 0) | (4 if weight else 0)
        nv.check(self.lib.casv_debug_contract(self.handle, flags, M, N, K, nv.ptr(A), nv.ptr(Bt), nv.ptr(bias), nv.ptr(C)))
        return C

    def debug_contract_tn(self, A, B, C, Mstore=None, colsum=None, accumulate=False, ordered=False):
        """Test support (casv_debug_contract_tn): C[:Mstore] (+)= A^T . B through the train step's weight-gradient dispatch, in
        place; colsum[:Mstore] += A.sum(0) when given.  A (K, M) and B (K, N) may be column windows of wider float32 arrays (row
        stride = lda / ldb), C (Mstore, N) one of a wider array too.  Returns the launch's (split, shares, nonempty_shares)."""
        def window(a, name):
            assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.ndim == 2 and a.strides[1] == 4, name
            return a.strides[0] // 4
        (K, M), N = A.shape, B.shape[1]
        Mstore = M if Mstore is None else int(Mstore)
        assert B.shape[0] == K and C.shape == (Mstore, N)
        lda, ldb, ldc = window(A, 'A'), window(B, 'B'), window(C, 'C')
        flags = (1 if accumulate else 0) | (2 if colsum is not None else 0) | (4 if ordered else 0)
        if colsum is not None:
            assert colsum.dtype == np.float32 and colsum.shape == (Mstore,) and colsum.flags.c_contiguous
        nv.check(self.lib.casv_debug_contract_tn(self.handle, flags, M, Mstore, N, K, nv.ptr(A), lda, nv.ptr(B), ldb, nv.ptr(C), ldc,
                                                 nv.ptr(colsum)))
        return self.stat('tn_split'), self.stat('tn_shares'), self.stat('tn_nonempty_shares')

    def debug_activation(self, which, x):
        """Test support (casv_debug_activation): which 'tanh' / 'sigmoid' on x (float32, any shape), or 'lstm_cell' on x (n, 5) =
        (z_i, z_f, z_g, z_o, c_prev) rows -> (n, 2) = (c, h), through the inline functions of csrc/common.h."""
        w = {'tanh': 0, 'sigmoid': 1, 'lstm_cell': 2}[which]
        x = nv.carray(x, np.float32)
        n = x.shape[0] if w == 2 else x.size
        assert w != 2 or x.shape == (n, 5)
        out = np.empty((n, 2) if w == 2 else x.shape, np.float32)
        nv.check(self.lib.casv_debug_activation(self.handle, w, n, nv.ptr(x), nv.ptr(out)))
        return out

    def debug_gemm_jobs(self, epi, jobs, step, step_by_ptr=False, acc=None, sums=None, ordered=False):
        """Test support (casv_debug_gemm_jobs): ONE batch of forward GEMM jobs (epi 0 plain, 1 fused LSTM cell) with the whole
        operand machinery of csrc/gemm_args.h, on host data.  A job is an object with the attributes M, N, Ktot, segs, c_in, zinit, Bt,
        bias, out, c_out, gates_out, out2, nact, nact_group, b_static, epi_plain; an input part (segment, c_in, zinit) has pool
        (slots, pool_rows, ld) float32, width, koff, rows, first, step_mul, step_add, skip_first; an output is (slots, ld, step_mul,
        step_add) or None (tests/lstm_gemm_cases.py builds them).  Returns (outputs, forms, launches): per job a dict name ->
        (slots, M, ld) float32 with every byte the launch did not store to still 0xFF, the bit mask of the GemmForms of the plan that
        ran, and the number of its launches.  acc (casv_debug_gemm_jobs_acc): per job an input part whose rows (width N) the job's
        accumulators start from, or None.  sums (casv_debug_gemm_jobs_sum): per job None or a dict of the train step's launch fields
        ksplit, kgroups, accumulate, out_zeroed (those left out are 0) and, with accumulate, C0 (M, N): what the addressed slot of
        `out` holds before the launch; ordered: the launch runs under ordered sums, as the deterministic train step's do.
        stat('gemm_jobs_shares') then tells the largest number of K shares of a launch of the plan."""
        keep, cjobs, results = [], (nv.DebugJob * len(jobs))(), []
        assert acc is None or sums is None
        assert sums is not None or not ordered
        csums = None if sums is None else (nv.DebugSum * len(jobs))()
        caccs = None if acc is None else (nv.DebugRows * len(jobs))()

        def arr(a, dtype):
            if a is None:
                return None
            a = nv.carray(a, dtype)
            keep.append(a)
            return a.ctypes.data

        def rows(dst, part):
            pool = nv.carray(part.pool, np.float32)
            assert pool.ndim == 3
            dst.slots, dst.pool_rows, dst.ld = pool.shape
            dst.pool, dst.rows, dst.first = arr(pool, np.float32), arr(part.rows, np.int32), arr(part.first, np.float32)
            assert part.rows is None or len(part.rows) == job.M
            assert part.first is None or np.shape(part.first) == (job.M, dst.ld)
            dst.width, dst.koff, dst.step_mul, dst.step_add, dst.skip_first = part.width, part.koff, part.step_mul, part.step_add, int(part.skip_first)

        def out(dst, spec, name, res):
            if spec is None:
                return
            slots, ld, mul, add = spec
            res[name] = np.empty((slots, job.M, ld), np.float32)
            dst.data, dst.slots, dst.ld, dst.step_mul, dst.step_add = res[name].ctypes.data, slots, ld, mul, add

        for cj, job in zip(cjobs, jobs):
            res = {}
            cj.M, cj.N, cj.Ktot, cj.nseg = job.M, job.N, job.Ktot, len(job.segs)
            assert 1 <= len(job.segs) <= 3 and np.shape(job.Bt) == (job.N, job.Ktot)
            for i, sg in enumerate(job.segs):
                rows(cj.a[i], sg)
            if job.c_in is not None:
                rows(cj.c_in, job.c_in)
            if job.zinit is not None:
                rows(cj.zinit, job.zinit)
            cj.Bt, cj.bias = arr(job.Bt, np.float32), arr(job.bias, np.float32)
            assert job.bias is None or np.shape(job.bias) == (job.N,)
            for name in ('out', 'c_out', 'gates_out', 'out2'):
                out(getattr(cj, name), getattr(job, name), name, res)
            if job.nact is not None:
                cj.nact, cj.nact_lines, cj.nact_group = arr(job.nact, np.int32), len(job.nact), job.nact_group
            cj.b_static, cj.epi_plain = int(job.b_static), int(job.epi_plain)
            results.append(res)
        if sums is not None:
            assert len(sums) == len(jobs)
            for cs, job, res, fields in zip(csums, jobs, results, sums):
                fields = dict(fields or {})
                c0 = fields.pop('C0', None)
                for name in ('ksplit', 'kgroups', 'accumulate', 'out_zeroed'):
                    setattr(cs, name, int(fields.pop(name, 0)))
                assert not fields, fields
                if c0 is not None:
                    slots, ld, mul, add = job.out
                    assert np.shape(c0) == (job.M, job.N) and 0 <= step * mul + add < slots
                    res['out'][step * mul + add, :, :job.N] = c0
            nv.check(self.lib.casv_debug_gemm_jobs_sum(self.handle, int(epi), len(jobs), cjobs, csums, int(bool(ordered)), int(step),
                                                       int(bool(step_by_ptr))))
        elif acc is not None:
            assert len(acc) == len(jobs)
            for ca, job, part in zip(caccs, jobs, acc):
                if part is not None:
                    rows(ca, part)
            nv.check(self.lib.casv_debug_gemm_jobs_acc(self.handle, int(epi), len(jobs), cjobs, caccs, int(step), int(bool(step_by_ptr))))
        else:
            nv.check(self.lib.casv_debug_gemm_jobs(self.handle, int(epi), len(jobs), cjobs, int(step), int(bool(step_by_ptr))))
        return results, self.stat('gemm_jobs_forms'), self.stat('gemm_jobs_launches')

    def debug_bwd_step(self, form, jobs, outputs=None):
        """Test support (casv_debug_bwd_step): ONE backward time step of 1 or 2 layers on host data; form 0 the fused launch, 1 the
        two launches.  A job is an object with the attributes rows, W, N, Bt (N, 4W), gates (rows, 4W), cell, dc_in (rows, W) and the
        optional inputs a, b, c, c_prev -- None or float32 arrays of `rows` rows whose row stride is the ld (a column window of a wider
        array: W columns are read) -- mask_a (W,) or None, and ld_out.  Returns per job a dict dz (rows + 1, 4W), dc (rows + 1, W), out
        (rows + 1, ld_out), every byte the launches did not store to still 0xFF (`outputs`: the arrays to fill instead of fresh ones)."""
        keep, cjobs, results = [], (nv.DebugBwdJob * len(jobs))(), []

        def dense(a):
            a = nv.carray(a, np.float32)
            keep.append(a)
            return a.ctypes.data

        def window(a, name):
            if a is None:
                return None, 0
            assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.ndim == 2 and a.strides[1] == 4 and a.strides[0] % 4 == 0, name
            keep.append(a)
            return a.ctypes.data, a.strides[0] // 4 if a.shape[0] > 1 else max(a.strides[0] // 4, a.shape[1])

        for i, (cj, job) in enumerate(zip(cjobs, jobs)):
            rows, W, N = int(job.rows), int(job.W), int(job.N)
            assert np.shape(job.Bt) == (N, 4 * W) and np.shape(job.gates) == (rows, 4 * W)
            assert np.shape(job.cell) == np.shape(job.dc_in) == (rows, W)
            cj.rows, cj.W, cj.N, cj.ld_out = rows, W, N, int(job.ld_out)
            cj.Bt, cj.gates, cj.cell, cj.dc_in = dense(job.Bt), dense(job.gates), dense(job.cell), dense(job.dc_in)
            cj.a, cj.lda = window(job.a, 'a')
            cj.b, cj.ldb = window(job.b, 'b')
            cj.c, cj.ldc = window(job.c, 'c')
            cj.c_prev, cj.ld_cprev = window(job.c_prev, 'c_prev')
            cj.mask_a = None if job.mask_a is None else dense(job.mask_a)
            res = outputs[i] if outputs is not None else {
                'dz': np.empty((rows + 1, 4 * W), np.float32), 'dc': np.empty((rows + 1, W), np.float32),
                'out': np.empty((rows + 1, max(int(job.ld_out), 1)), np.float32)}
            for name in ('dz', 'dc', 'out'):
                assert res[name].dtype == np.float32 and res[name].flags.c_contiguous
            cj.dz, cj.dc, cj.out = res['dz'].ctypes.data, res['dc'].ctypes.data, res['out'].ctypes.data
            results.append(res)
        nv.check(self.lib.casv_debug_bwd_step(self.handle, int(form), len(jobs), cjobs))
        return results

    def alignments_sparse(self, rows, steps, K=None):
        """Window form of the last decode call's soft alignments: (lo int32 (rows, S), w float32 (rows, S, K))."""
        K = int(K or 2 * self.window_width + 1)
        lo = np.empty((rows, steps), np.int32)
        w = np.empty((rows, steps, K), np.float32)
        nv.check(self.lib.casv_get_alignments_sparse(self.handle, K, nv.ptr(lo), nv.ptr(w)))
        return lo, w

    # -- result records on the device (sharding.py) ------------------------------------------
    def records_reset(self, rows, steps):
        """A zeroed device buffer of `rows` result records of `steps` steps (2*steps+4 int32 each)."""
        self._rec_shape = (int(rows), 2 * int(steps) + 4)
        nv.check(self.lib.casv_records_reset(self.handle, int(rows), int(steps)))

    def records_append(self, row_offset):
        """Pack the best result of every line of the last decode call into records [row_offset, row_offset + B)."""
        nv.check(self.lib.casv_records_append(self.handle, int(row_offset)))

    def records_read(self):
        out = np.empty(self._rec_shape, np.int32)
        nv.check(self.lib.casv_records_read(self.handle, nv.ptr(out)))
        return out

    def records_device_ptr(self):
        """(device address, bytes) of the record buffer, after the handle's stream has drained."""
        p, n = c_void_p(), c_int64()
        nv.check(self.lib.casv_records_device_ptr(self.handle, byref(p), byref(n)))
        return p.value, n.value

    def stat(self, key):
        v = c_int64()
        nv.check(self.lib.casv_get_stat(self.handle, key.encode(), byref(v)))
        return v.value

    def synchronize(self):
        nv.check(self.lib.casv_synchronize(self.handle))
