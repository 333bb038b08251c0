"""lm_predict without a GPU: the oracle's restatement of the LM output (tests/lm_oracle.py) against an independent torch
LSTMCell stack, its NaN rows, and the facade's switch (configure() refuses the flag, a beam decode after it reads it)."""
import numpy as np
import pytest
import torch

from oracle import ModelConfig, make_weights, make_lines, vectorize_lines
from oracle.decode import OracleModel, decode_sequence_beam
from tests.lm_oracle import lm_step, decode_sequence_beam_lm


def _torch_lm(cfg, w, p_in, states):
    """The LM output by torch.nn.LSTMCell: lower layers on the embedded input, the top cell on [x | 0] (the zero context)."""
    d, W = cfg.depth, cfg.width
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))

    def cell(x, h, c, n):
        K, R, b = w['dec%d_K' % n], w['dec%d_R' % n], w['dec%d_b' % n]
        m = torch.nn.LSTMCell(K.shape[0], W).double()
        with torch.no_grad():              # Keras (in, 4W) gate blocks i, f, c, o == torch's i, f, g, o rows
            m.weight_ih.copy_(t(K).T)
            m.weight_hh.copy_(t(R).T)
            m.bias_ih.copy_(t(b))
            m.bias_hh.zero_()
        with torch.no_grad():
            return m(x, (h, c))

    x = t(p_in) @ t(w['E'])
    for n in range(1, d):
        x, _ = cell(x, t(states[2 * n - 2]), t(states[2 * n - 1]), n)
    ctx_w = w['dec%d_K' % d].shape[0] - x.shape[1]
    h, _ = cell(torch.cat([x, torch.zeros(x.shape[0], ctx_w, dtype=x.dtype)], 1), t(states[2 * d - 2]), t(states[2 * d - 1]), d)
    return torch.softmax(h @ t(w['E']).T, dim=1).numpy()


def _rows(cfg, w, R, T, rng, off_line=()):
    """R decoder rows: perturbed states, random input distributions, alignments over a few live positions; rows in `off_line`
    have their alignment mass far beyond the line end (t' > T - 1 + window: the window is empty)."""
    V, W = cfg.voc_size, cfg.width
    states = [rng.normal(0, 0.3, (R, W)) for _ in range(2 * cfg.depth)]
    logits = rng.normal(0, 2.0, (R, V))
    p_in = np.exp(logits - logits.max(axis=1, keepdims=True))
    p_in /= p_in.sum(axis=1, keepdims=True)
    a = np.zeros((R, T))
    pos = rng.integers(0, T - 2, R)
    for k in range(3):
        a[np.arange(R), pos + k] = rng.random(R) + 0.1
    a /= a.sum(axis=1, keepdims=True)
    for r in off_line:
        a[r] = 0
        a[r, T - 1] = 4.0
    enc = rng.normal(0, 0.5, (R, T, w['att_U'].shape[0]))
    return p_in, states + [a], enc


@pytest.mark.parametrize('depth', [1, 2, 4])
def test_lm_step_equals_a_torch_lstm_cell_on_a_zero_context(depth):
    cfg = ModelConfig(depth=depth, width=32, voc_size=24)
    w = make_weights(cfg, dtype=np.float64, emb_scale=8.0)
    m = OracleModel(cfg, w)
    p_in, states, enc = _rows(cfg, w, 12, 9, np.random.default_rng(depth))
    got = lm_step(m, p_in, enc, states)
    want = _torch_lm(cfg, w, p_in, states)
    assert np.isfinite(got).all()
    assert np.allclose(got, want, rtol=1e-9, atol=1e-12)
    # ... and it is not the decoder's output: the context matters there
    dec, _ = m.step(p_in, enc, states)
    assert not np.allclose(got, dec, rtol=1e-3)


def test_lm_rows_are_nan_where_the_window_falls_off_the_line():
    cfg = ModelConfig(depth=2, width=32, voc_size=24)
    w = make_weights(cfg, dtype=np.float64, emb_scale=8.0)
    m = OracleModel(cfg, w)
    off = (1, 4, 5)
    p_in, states, enc = _rows(cfg, w, 8, 4, np.random.default_rng(3), off_line=off)
    with np.errstate(invalid='ignore'):
        got = lm_step(m, p_in, enc, states)
        dec, _ = m.step(p_in, enc, states)
    nan_lm, nan_dec = np.isnan(got).all(axis=1), np.isnan(dec).all(axis=1)
    assert list(np.nonzero(nan_lm)[0]) == list(off)
    assert np.array_equal(nan_lm, nan_dec)
    assert np.isfinite(got[~nan_lm]).all()
    # an energy of 0 (b_v far below) empties the LM's normalisation even where the window is live: NaN rows everywhere
    w0 = dict(w)
    w0['att_bv'] = np.array([-1e4])
    with np.errstate(invalid='ignore', over='ignore'):
        assert np.isnan(lm_step(OracleModel(cfg, w0), p_in, enc, states)).all()


def test_the_lm_rated_search_takes_other_decisions():
    """The restated search is the plain one but for the cost: on the model of the GPU tests' short lines it returns other
    results (so a device test that compares with it shows the switch acts)."""
    cfg = ModelConfig(depth=2, width=64, voc_size=64)
    w = make_weights(cfg, emb_scale=14.0)
    m = OracleModel(cfg, w, batch_size=4)
    lines, _ = make_lines(6, 12, 13, voc_size=64)
    enc_in, _, _, _ = vectorize_lines(m, lines, [[] for _ in lines])
    enc = m.encode(enc_in)
    differ = 0
    for j in range(len(lines)):
        a = next(decode_sequence_beam(m, source_seq=enc_in[j], encoder_outputs=[e[j:j + 1] for e in enc]), None)
        b = next(decode_sequence_beam_lm(m, source_seq=enc_in[j], encoder_outputs=[e[j:j + 1] for e in enc]), None)
        if a is None or b is None:          # (no finished hypothesis: the generator raises StopIteration, s2s:826)
            differ += (a is None) != (b is None)
            continue
        differ += a[0] != b[0] or abs(a[2] - b[2]) > 1e-6
        # probabilities stay the decoder's: a shared prefix has the same ones
        n = 0
        while n < min(len(a[0]), len(b[0])) and a[0][n] == b[0][n]:
            n += 1
        assert np.allclose(a[1][:n], b[1][:n])
    assert differ >= 1


class _StubEngine(object):
    """Records what the facade asks of the engine (no device needed)."""
    calls = []

    def __init__(self, depth, width, voc_size, **kw):
        self.depth, self.width, self.voc_size, self.T, self.B = depth, width, voc_size, 0, 0
        self.options = {}

    def set_weights(self, w):
        pass

    def set_option(self, key, value):
        self.options[key] = value

    def encode(self, idx, val=None, src_rej=None):
        self.B, self.T = idx.shape[:2]

    def set_encoder_outputs(self, enc_out, states, a0=None, src_rej=None):
        self.B, self.T = np.asarray(enc_out).shape[:2]

    def decode_beam(self, max_results=1, want_align=False, **kw):
        _StubEngine.calls.append(('decode_beam', dict(self.options)))
        n, S = self.B * max_results, 2 * self.T
        return {'idx': np.ones((n, S), np.int32), 'prob': np.ones((n, S), np.float32), 'len': np.zeros(n, np.int32),
                'score': np.zeros(n), 'rej': -np.ones((n, S), np.int32), 'align': None, 'align_sparse': None,
                'n_found': np.zeros(self.B, np.int32), 'n_steps': np.zeros(self.B, np.int32)}

    def decoder_step(self, line, p_in, states, a_in):
        _StubEngine.calls.append(('decoder_step', None))
        return p_in, list(states) + [a_in]

    def decoder_step_lm(self, line, p_in, states, a_in):
        _StubEngine.calls.append(('decoder_step_lm', None))
        return p_in, p_in * 0.5, list(states) + [a_in]

    def close(self):
        pass


def _stub_facade(monkeypatch):
    from cor_asv_ann_amd import seq2seq
    monkeypatch.setattr(seq2seq, 'HipEngine', _StubEngine)
    _StubEngine.calls = []
    s2s = seq2seq.Sequence2Sequence()
    s2s.depth, s2s.width, s2s.batch_size = 2, 32, 4
    s2s.mapping = ({'': 0, '\n': 1, 'a': 2, 'b': 3}, {0: '', 1: '\n', 2: 'a', 3: 'b'})
    s2s.voc_size = 4
    return s2s


def test_configure_refuses_the_flag_and_a_beam_decode_after_it_reads_it(monkeypatch):
    s2s = _stub_facade(monkeypatch)
    s2s.lm_predict = True
    with pytest.raises(NotImplementedError, match='lm_predict'):
        s2s.configure()
    s2s.lm_predict = False
    s2s.configure()
    s2s.status = 2
    src = np.zeros((3, 4), np.float32)
    src[np.arange(3), [2, 3, 1]] = 1
    list(s2s.decode_sequence_beam(source_seq=src))
    s2s.lm_predict = True                       # honoured from the next decode on, like rejection_threshold
    list(s2s.decode_sequence_beam(source_seq=src))
    s2s.correct_lines(['ab\n'], fast=False, greedy=False)
    s2s.lm_predict = False
    s2s.correct_lines(['ab\n'], fast=False, greedy=False)
    seen = [opts['lm_predict'] for what, opts in _StubEngine.calls if what == 'decode_beam']
    assert seen == [0, 1, 1, 0]


def test_decoder_model_returns_the_lm_scores_second(monkeypatch):
    s2s = _stub_facade(monkeypatch)
    s2s.configure()
    s2s.status = 2
    R, T, W = 3, 5, s2s.width
    p = np.full((R, 1, 4), 0.25, np.float32)
    states = [np.zeros((R, W), np.float32)] * 4 + [np.zeros((R, T), np.float32)]
    inputs = [p, np.zeros((1, T, W), np.float32)] + states
    out = s2s.decoder_model.predict_on_batch(inputs)
    assert len(out) == 1 + 5 and _StubEngine.calls[-1][0] == 'decoder_step'
    s2s.lm_predict = True
    out = s2s.decoder_model.predict_on_batch(inputs)
    assert len(out) == 2 + 5 and _StubEngine.calls[-1][0] == 'decoder_step_lm'
    assert out[0].shape == out[1].shape == (R, 1, 4)
    assert np.allclose(out[1], 0.5 * out[0])


def test_the_beam_memory_budget_counts_the_lm_scratch(monkeypatch):
    s2s = _stub_facade(monkeypatch)
    s2s.configure()
    s2s.status = 2
    lines = ['ab\n'] * 6
    prepared = s2s._prepare_lines(lines, None)
    B, T = prepared[0].shape[:2]
    children = min(s2s.beam_width_in, s2s.voc_size) + 1
    per_line = 2 * T * s2s.batch_size * (((2 * s2s.depth + 1) * s2s.width + s2s.voc_size + 32 + T) * 4 + 60 * children)
    # a budget that holds exactly two lines without the LM's scratch: two lines per call, and one with it
    monkeypatch.setenv('CASV_BEAM_MEMORY_GB', repr(2 * per_line / 2 ** 30))
    _, out = s2s._decode_prepared(prepared, False, False, False, [True] * B)
    assert [len(rows) for rows, _, _ in out] == [2, 2, 2]
    s2s.lm_predict = True
    _, out = s2s._decode_prepared(prepared, False, False, False, [True] * B)
    assert [len(rows) for rows, _, _ in out] == [1] * 6
