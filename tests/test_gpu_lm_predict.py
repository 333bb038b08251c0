"""lm_predict on a real MI355X: casv_decoder_step_lm against the oracle's LM step (tests/lm_oracle.py), the LM-rated beam search
against the restated search, and the invariances of the search with the option on.  Tolerances as tests/test_gpu_parity.py:
indices, strings, lengths exact; probabilities rtol 2e-4 + atol 2e-6; decisions compared where the oracle's own fp32 and fp64
searches agree."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import ModelConfig, make_weights, make_lines, vectorize_lines
from oracle.decode import OracleModel
from tests.golden.make_golden import CASES
from tests.lm_oracle import lm_step, decode_sequence_beam_lm

RT, AT = 2e-4, 2e-6


def _engine(cfg, weights):
    from cor_asv_ann_amd.engine import HipEngine
    eng = HipEngine(cfg.depth, cfg.width, cfg.voc_size)
    eng.set_weights(weights)
    return eng


def _facade(cfg, weights, mapping, N=4):
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence
    s2s = Sequence2Sequence()
    s2s.depth, s2s.width, s2s.batch_size = cfg.depth, cfg.width, N
    s2s.mapping, s2s.voc_size = mapping, cfg.voc_size
    s2s.configure()
    s2s.set_weights(weights)
    s2s.status = 2
    return s2s


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _step_rows(enc, B, N, rng):
    """R = B * N rows: the lines' encoder states, perturbed."""
    R = B * N
    line = np.repeat(np.arange(B), N).astype(np.int32)
    states = [np.repeat(s, N, axis=0) + rng.normal(0, 0.1, (R, s.shape[1])).astype(np.float32) for s in enc[1:-1]]
    return line, states, R


def _check_step(cfg, weights, B, N, L, seed, rng):
    V, T = cfg.voc_size, L + 1
    lines, idx = make_lines(B, L, seed, voc_size=V)
    om = OracleModel(cfg, weights)
    enc_in, _, _, _ = vectorize_lines(om, lines, [[] for _ in lines])
    enc = om.encode(enc_in)
    eng = _engine(cfg, weights)
    eng.set_encoder_outputs(enc[0], enc[1:-1])
    line, states, R = _step_rows(enc, B, N, rng)
    logits = rng.normal(0, 2.0, (R, V)).astype(np.float32)
    p_in = np.exp(logits - logits.max(axis=1, keepdims=True))
    p_in /= p_in.sum(axis=1, keepdims=True)
    a_in = np.zeros((R, T), np.float32)
    pos = rng.integers(0, T - 2, R)
    for k in range(3):
        a_in[np.arange(R), pos + k] = rng.random(R).astype(np.float32) + 0.1
    a_in /= a_in.sum(axis=1, keepdims=True)
    off = rng.choice(R, size=max(2, R // 64), replace=False)
    a_in[off] = 0
    a_in[off, T - 1] = 4.0                      # t' far beyond the line: the window is empty
    probs, st = eng.decoder_step(line, p_in, states, a_in)
    probs2, lm, st2 = eng.decoder_step_lm(line, p_in, states, a_in)
    eng.close()
    # the decoder's outputs are casv_decoder_step's, bit for bit
    assert np.array_equal(_bits(probs), _bits(probs2))
    for x, y in zip(st, st2):
        assert np.array_equal(_bits(x), _bits(y))
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        want = lm_step(om, p_in, enc[0][line], states + [a_in])
    nan_got, nan_want = np.isnan(lm), np.isnan(want)
    assert np.array_equal(nan_got, nan_want)
    assert nan_got.all(axis=1)[off].all() and nan_got.any(axis=1).sum() == len(off)
    ok = ~nan_want.any(axis=1)
    assert np.allclose(lm[ok], want[ok], rtol=RT, atol=AT)
    assert not np.allclose(lm[ok], probs[ok], rtol=1e-2)        # the LM is not the decoder


@pytest.mark.parametrize('name', ['c1_d1_w128_peaky', 'd2_w128_v64', 'd4_w128_v256', 'd2_w64_v96'])
def test_decoder_step_lm_equals_the_oracle(name):
    d, W, V, B, L, seed, es, N = CASES[name]
    cfg = ModelConfig(depth=d, width=W, voc_size=V)
    _check_step(cfg, make_weights(cfg, emb_scale=es), B, N, L, seed, np.random.default_rng(d * 1000 + V))


def test_decoder_step_lm_at_full_width_rows():
    """R = 8192 rows (1024 lines x 8 hypotheses) at depth 4, width 512, V 256: the LM job beside the top cell at the tile shapes
    of the metric's launches."""
    cfg = ModelConfig(depth=4, width=512, voc_size=256)
    _check_step(cfg, make_weights(cfg, emb_scale=32.0), 1024, 8, 12, 103, np.random.default_rng(11))


def _texts(om, res, B):
    i_c = om.mapping[1]
    return [''.join(i_c[int(c)] for c in res['idx'][j, :int(res['len'][j])]) for j in range(B)]


def _oracle_lm(cfg, weights, lines, N, dtype):
    w = {k: v.astype(dtype) for k, v in weights.items()}
    om = OracleModel(cfg, w, batch_size=N)
    enc_in, _, _, _ = vectorize_lines(om, lines, [[] for _ in lines])
    enc = om.encode(enc_in)
    out = []
    for j in range(len(lines)):
        try:
            out.append(next(decode_sequence_beam_lm(om, source_seq=enc_in[j], encoder_outputs=[e[j:j + 1] for e in enc])))
        except StopIteration:
            out.append(None)
        except IndexError:          # source_seq[source_pos] beyond the line (reference quirk 6): pins nothing
            out.append(False)
    return out


SHORT = {'d2_w64_v64': (2, 64, 64, 14.0, 4, 12, 13), 'd1_w128_v256': (1, 128, 256, 14.0, 8, 12, 101),
         'd4_w128_v256': (4, 128, 256, 64.0, 8, 12, 101)}


@pytest.mark.parametrize('name', list(SHORT))
def test_lm_beam_equals_the_oracle_on_short_lines(name):
    d, W, V, es, N, L, seed = SHORT[name]
    cfg = ModelConfig(depth=d, width=W, voc_size=V)
    weights = make_weights(cfg, emb_scale=es)
    lines, idx = make_lines(6, L, seed, voc_size=V)
    B = len(lines)
    o32 = _oracle_lm(cfg, weights, lines, N, np.float32)
    o64 = _oracle_lm(cfg, weights, lines, N, np.float64)
    eng = _engine(cfg, weights)
    eng.encode(idx)
    plain = eng.decode_beam(batch_size=N)
    eng.set_option('lm_predict', 1)
    res = eng.decode_beam(batch_size=N)
    eng.close()
    om = OracleModel(cfg, weights)
    got, got_plain = _texts(om, res, B), _texts(om, plain, B)
    pinned = 0
    for j in range(B):
        a, b = o32[j], o64[j]
        if a is False or b is False or (a is None) != (b is None) or (a is not None and a[0] != b[0]):
            continue                                    # the oracle itself does not pin this line
        pinned += 1
        if a is None:
            assert res['n_found'][j] == 0, j
            continue
        n = len(a[0])
        assert got[j] == a[0] and int(res['len'][j]) == n, j
        assert list(res['rej'][j, :n]) == list(a[4]), j
        assert np.allclose(res['prob'][j, :n], np.asarray(a[1], np.float32), rtol=RT, atol=AT), j
        assert abs(res['score'][j] - a[2]) <= RT * abs(a[2]) + 1e-5, j
    assert pinned >= 4
    assert any(x != y for x, y in zip(got, got_plain)) or not np.array_equal(res['score'], plain['score'])


def test_lm_beam_at_the_bench_shape_agrees_with_the_oracle_like_its_own_fp64_run():
    """configs[2]'s shape (depth 4, width 512, V 256, N = 8) on the first 100-character lines of its batch, with flat weights
    (emb_scale 4: with the bench's peaky ones no LM-rated search of these lines finishes within its 202 steps, so there would be
    nothing to compare).  A 200-step search amplifies rounding: as in test_c3_bench_batch_..., the decisions
    may leave the fp32 oracle on at most 3x as many lines as its own fp64 run does (plus one: four lines are few), and where all
    three agree the per-line maximum relative probability error and the score error stay within 3x the fp64 run's (or the usual
    tolerance)."""
    cfg = ModelConfig(depth=4, width=512, voc_size=256)
    weights = make_weights(cfg, emb_scale=4.0)
    lines, idx = make_lines(1024, 100, 103, voc_size=256)
    lines, idx = lines[:4], idx[:4]
    B = len(lines)
    o32 = _oracle_lm(cfg, weights, lines, 8, np.float32)
    o64 = _oracle_lm(cfg, weights, lines, 8, np.float64)
    eng = _engine(cfg, weights)
    eng.encode(idx)
    eng.set_option('lm_predict', 1)
    res = eng.decode_beam(batch_size=8)
    eng.close()
    got = _texts(OracleModel(cfg, weights), res, B)
    keep = [j for j in range(B) if o32[j] is not False and o64[j] is not False]
    assert len(keep) >= 3
    o32, o64, got, B = [o32[j] for j in keep], [o64[j] for j in keep], [got[j] for j in keep], len(keep)
    res = {k: res[k][keep] for k in ('prob', 'score', 'n_found')}
    t32 = [a[0] if a else None for a in o32]
    t64 = [a[0] if a else None for a in o64]
    dev = sum(1 for j in range(B) if (got[j] if res['n_found'][j] else None) != t32[j])
    d64 = sum(1 for j in range(B) if t64[j] != t32[j])
    same = [j for j in range(B) if t32[j] and got[j] == t32[j] == t64[j]]
    e_dev, e_64, s_dev, s_64 = [], [], [], []
    for j in same:
        n = len(t32[j])
        p32, p64 = np.asarray(o32[j][1], np.float64), np.asarray(o64[j][1], np.float64)
        e_dev.append(np.max(np.abs(res['prob'][j, :n] - p32) / np.maximum(p32, 1e-6)))
        e_64.append(np.max(np.abs(p64 - p32) / np.maximum(p32, 1e-6)))
        s_dev.append(abs(res['score'][j] - o32[j][2]))
        s_64.append(abs(o64[j][2] - o32[j][2]))
    print('lm beam at the bench shape, %d lines: decisions differ from the fp32 oracle on %d (fp64 oracle: %d); equal on %d: '
          'probability errors %s (fp64 oracle %s), score errors %s (%s)' % (B, dev, d64, len(same), e_dev, e_64, s_dev, s_64))
    assert dev <= 3 * d64 + 1 and len(same) >= 2
    for ed, e6, sd, s6 in zip(e_dev, e_64, s_dev, s_64):
        assert ed <= max(3 * e6, 1e-3)
        assert sd <= max(3 * s6, 1e-4)


def _same(a, b):
    for k in ('idx', 'len', 'rej', 'n_found', 'n_steps'):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a['score'].view(np.int64), b['score'].view(np.int64))
    assert np.array_equal(_bits(a['prob']), _bits(b['prob']))


def _pick(res, rows):
    out = {k: res[k][rows] for k in ('idx', 'len', 'rej', 'score', 'prob', 'n_found', 'n_steps')}
    return out


def test_lm_beam_bits_do_not_depend_on_batch_order_launch_form_or_history():
    cfg = ModelConfig(depth=2, width=128, voc_size=64)
    weights = make_weights(cfg, emb_scale=16.0)
    _, idx = make_lines(600, 20, 3, voc_size=64)
    eng = _engine(cfg, weights)
    eng.encode(idx)
    default = eng.decode_beam(batch_size=4)
    eng.set_option('lm_predict', 1)
    full = eng.decode_beam(batch_size=4)
    assert not (np.array_equal(full['idx'], default['idx']) and np.array_equal(full['score'], default['score']))
    for j in (0, 17, 599):                                  # one line alone
        eng.encode(idx[j:j + 1])
        _same(_pick(full, [j]), eng.decode_beam(batch_size=4))
    order = np.random.default_rng(2).permutation(600)      # another order
    eng.encode(idx[order])
    _same(_pick(full, order), eng.decode_beam(batch_size=4))
    eng.encode(idx[:9])
    eager = eng.decode_beam(batch_size=4)
    eng.set_option('graph', 1)                              # graph replay
    _same(eager, eng.decode_beam(batch_size=4))
    _same(eager, eng.decode_beam(batch_size=4))
    eng.set_option('graph', 0)
    eng.set_option('lm_predict', 0)                         # back to the default bits
    eng.encode(idx)
    _same(default, eng.decode_beam(batch_size=4))
    eng.close()


def test_lm_beam_chunked_equals_unchunked_and_greedy_ignores_the_switch(monkeypatch):
    cfg = ModelConfig(depth=2, width=64, voc_size=64)
    weights = make_weights(cfg, emb_scale=14.0)
    om = OracleModel(cfg, weights)
    lines, _ = make_lines(12, 14, 21, voc_size=64)
    s2s = _facade(cfg, weights, om.mapping, N=4)

    def greedy_run(fast):
        try:
            return s2s.correct_lines(lines, fast=fast, greedy=True)
        except ValueError as err:           # (index 0 won a step of decode_sequence_greedy: seq2seq.py:1334-1335)
            return str(err)
    greedy = [greedy_run(f) for f in (True, False)]
    plain = s2s.correct_lines(lines, fast=False, greedy=False)
    s2s.lm_predict = True
    whole = s2s.correct_lines(lines, fast=False, greedy=False)
    assert whole[0] != plain[0] or whole[2] != plain[2]
    monkeypatch.setenv('CASV_BEAM_MEMORY_GB', '0.0001')       # a few lines per call
    chunked = s2s.correct_lines(lines, fast=False, greedy=False)
    monkeypatch.delenv('CASV_BEAM_MEMORY_GB')
    assert chunked[0] == whole[0] and chunked[2] == whole[2]
    for a, b in zip(chunked[1], whole[1]):
        assert np.array_equal(_bits(a), _bits(b))
    for f, want in zip((True, False), greedy):           # the greedy decodes do not use the LM
        got = greedy_run(f)
        if isinstance(want, str):
            assert got == want
            continue
        assert got[0] == want[0] and got[2] == want[2]
        for a, b in zip(got[1], want[1]):
            assert np.array_equal(_bits(a), _bits(b))


def test_decoder_model_returns_scores_then_lm_scores_then_states():
    cfg = ModelConfig(depth=2, width=64, voc_size=64)
    weights = make_weights(cfg, emb_scale=14.0)
    om = OracleModel(cfg, weights)
    lines, _ = make_lines(3, 10, 5, voc_size=64)
    enc_in, _, _, _ = vectorize_lines(om, lines, [[] for _ in lines])
    s2s = _facade(cfg, weights, om.mapping)
    enc = s2s.encoder_model.predict_on_batch(enc_in)
    p = np.zeros((3, 1, 64), np.float32)
    inputs = [p, enc[0]] + enc[1:]
    base = s2s.decoder_model.predict_on_batch(inputs)
    s2s.lm_predict = True
    out = s2s.decoder_model.predict_on_batch(inputs)
    assert len(out) == len(base) + 1
    assert np.array_equal(_bits(out[0]), _bits(base[0]))
    for x, y in zip(out[2:], base[1:]):
        assert np.array_equal(_bits(x), _bits(y))
    want = lm_step(om, p[:, 0], enc[0], list(enc[1:]))
    assert out[1].shape == (3, 1, 64)
    assert np.allclose(out[1][:, 0], want, rtol=RT, atol=AT)
