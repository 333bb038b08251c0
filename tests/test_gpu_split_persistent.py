"""The persistent encoder in the split arithmetic (csrc/persist_split.hip: the whole encoder recurrence of a small batch in one
launch on v_mfma_f32_32x32x16_bf16 with bf16x3-split operands) against the per-step split launches -- bit for bit -- through
the C ABI: encoder outputs, final states and everything a beam search returns.  The option "persistent" decides the form,
the statistic "encoder_persistent" tells which one ran."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import ModelConfig, make_weights

BEAM_KEYS = ('idx', 'prob', 'score', 'len', 'align', 'rej', 'n_found', 'n_steps')


def _engine(cfg, weights, **kw):
    from cor_asv_ann_amd.engine import HipEngine
    eng = HipEngine(cfg.depth, cfg.width, cfg.voc_size, residual_connections=cfg.residual_connections,
                    bridge_dense=cfg.bridge_dense, deep_bidirectional_encoder=cfg.deep_bidirectional_encoder, **kw)
    eng.set_weights(weights)
    return eng


def _lines(B, T, V, seed, alts=3):
    """B confusion-network lines of mixed length on T positions: up to `alts` alternatives per position (-1 = empty slot),
    confidences that sum to at most 1, the end-of-line character (index 1) last, nothing behind it.  Line 0 has the full length
    T, line 1 (if there is one) length 1 -- the end of line alone."""
    rng = np.random.default_rng(seed)
    idx = np.full((B, T, alts), -1, np.int32)
    val = np.zeros((B, T, alts), np.float32)
    for j in range(B):
        n = T if j == 0 else 1 if j == 1 else int(rng.integers(1, T + 1))
        for t in range(n - 1):
            k = int(rng.choice([1, 2, 3][:alts], p=np.array([0.60, 0.28, 0.12][:alts]) / sum([0.60, 0.28, 0.12][:alts])))
            idx[j, t, :k] = rng.choice(np.arange(2, V), size=k, replace=False)
            val[j, t, :k] = np.sort(rng.dirichlet(np.ones(k) * 0.7) * rng.uniform(0.7, 1.0))[::-1]
        idx[j, n - 1, 0] = 1
        val[j, n - 1, 0] = 1.0
    return idx, val


def _leg(eng, persistent, idx, val, N, search=True):
    """One pass in the form `persistent`: (encoder outputs + final states, search results, the statistic behind each)."""
    eng.set_option('persistent', persistent)
    eng.encode(idx, val)
    enc, states = eng.encoder_outputs()
    st_enc = eng.stat('encoder_persistent')
    out = [enc] + list(states)
    st_beam = None
    if search:
        eng.encode(idx, val)                       # (a fresh encoding: the search runs its own encoder pass)
        res = eng.decode_beam(batch_size=N, want_align=True, rejection_threshold=0.5)
        st_beam = eng.stat('encoder_persistent')
        out += [res[k] for k in BEAM_KEYS]
    return out, st_enc, st_beam


def _same(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), (what, k, int((x != y).sum()))


SHAPES = {
    # name: depth, width, V, lines, positions, hypotheses, emb_scale, flags
    'page': (2, 512, 640, 40, 61, 256, 128.0, {}),
    'depth1': (1, 128, 64, 20, 15, 8, 16.0, {}),                 # attended width 2W
    'depth4_b11': (4, 512, 256, 11, 20, 8, 64.0, {}),
    'width100': (2, 100, 96, 19, 14, 8, 12.0, {}),               # dead-unit padding to 128
    'b1': (2, 64, 50, 1, 10, 4, 8.0, {}),
    'b32': (2, 64, 50, 32, 10, 4, 8.0, {}),
    'b33': (2, 64, 50, 33, 10, 4, 8.0, {}),
    'b64': (2, 64, 50, 64, 10, 4, 8.0, {}),
    'b512': (2, 64, 50, 512, 10, 4, 8.0, {}),
    'depth3': (3, 96, 100, 21, 12, 8, 10.0, {}),
    'bridge': (2, 64, 48, 21, 12, 8, 8.0, dict(bridge_dense=True)),
}


@pytest.mark.parametrize('arithmetic', [2, 1])
@pytest.mark.parametrize('name', list(SHAPES))
def test_persistent_split_encoder_equals_the_per_step_one_bit_for_bit(name, arithmetic):
    d, W, V, B, T, N, es, flags = SHAPES[name]
    cfg = ModelConfig(depth=d, width=W, voc_size=V, **flags)
    weights = make_weights(cfg, emb_scale=es)
    idx, val = _lines(B, T, V, 1000 + B + T)
    if name == 'width100':                         # through the facade, whose engine pads the width with dead units
        from cor_asv_ann_amd.seq2seq import Sequence2Sequence
        from cor_asv_ann_amd.synthetic import make_vocabulary
        s2s = Sequence2Sequence()
        s2s.depth, s2s.width, s2s.batch_size = d, W, N
        s2s.mapping, s2s.voc_size = make_vocabulary(V), V
        s2s.configure()
        s2s.set_weights(weights)
        s2s.status = 2
        eng = s2s._require_engine()
        assert eng.pwidth == 128
    else:
        eng = _engine(cfg, weights)
    eng.set_option('arithmetic', arithmetic)
    step, s_enc0, s_beam0 = _leg(eng, 0, idx, val, N)
    pers, s_enc1, s_beam1 = _leg(eng, 1, idx, val, N)
    assert (s_enc0, s_beam0) == (0, 0), 'persistent = 0 is the per-step form'
    assert (s_enc1, s_beam1) == (1, 1), 'persistent = 1 is one persistent launch'
    _same(step, pers, name)
    # an encoding that is reused is nobody's pass
    eng.encoder_outputs()
    assert eng.stat('encoder_persistent') == 0
    eng.close()


def test_default_form():
    """"persistent" = -1: the search's encoder pass is the persistent launch up to the row limit and where the topology has that
    form; the chain arithmetic's entry points keep their own persistent encoder."""
    cfg = ModelConfig(depth=2, width=128, voc_size=64)
    weights = make_weights(cfg, emb_scale=16.0)
    eng = _engine(cfg, weights)
    idx, val = _lines(40, 16, 64, 7)
    eng.encode(idx, val)
    small = eng.decode_beam(batch_size=4)
    assert eng.stat('encoder_persistent') == 1
    big_idx, big_val = _lines(600, 16, 64, 8)          # above the row limit (and above the 512 rows of the chain kernel's)
    eng.encode(big_idx, big_val)
    eng.decode_beam(batch_size=4)
    assert eng.stat('encoder_persistent') == 0
    eng.set_option('persistent', 0)
    eng.encode(idx, val)
    step = eng.decode_beam(batch_size=4)
    assert eng.stat('encoder_persistent') == 0
    _same([small[k] for k in BEAM_KEYS if small[k] is not None], [step[k] for k in BEAM_KEYS if step[k] is not None], 'default form')
    # a greedy decode on a default handle: the chain arithmetic's persistent encoder, as before
    g = {}
    for p in (-1, 0):
        eng.set_option('persistent', p)
        eng.encode(idx, val)
        g[p] = eng.decode_greedy(mode=0, want_align=True)
        assert eng.stat('encoder_persistent') == (1 if p else 0)
    _same([g[-1][k] for k in range(4)], [g[0][k] for k in range(4)], 'greedy')
    eng.close()
    for flags, d in ((dict(residual_connections=True), 3), (dict(deep_bidirectional_encoder=True), 2)):
        cfg = ModelConfig(depth=d, width=64, voc_size=48, **flags)
        eng = _engine(cfg, make_weights(cfg, emb_scale=8.0))
        idx, val = _lines(12, 9, 48, 9)
        for p in (-1, 1):
            eng.set_option('persistent', p)
            eng.encode(idx, val)
            eng.decode_beam(batch_size=4)
            assert eng.stat('encoder_persistent') == 0, (flags, p)
        eng.close()


def test_never_by_batch():
    """The page's 40 lines searched alone (persistent encoder) and as lines 300..339 of a batch above the row limit (per-step
    launches): the same bits per line.  (16 hypotheses per line instead of the page's 256: the big batch's state stores grow
    with lines x hypotheses x steps.)"""
    d, W, V, B, T, N, es, _ = SHAPES['page']
    cfg = ModelConfig(depth=d, width=W, voc_size=V)
    eng = _engine(cfg, make_weights(cfg, emb_scale=es))
    idx, val = _lines(B, T, V, 1000 + B + T)
    N = 16
    eng.encode(idx, val)
    alone = eng.decode_beam(batch_size=N, want_align=True, rejection_threshold=0.5)
    assert eng.stat('encoder_persistent') == 1
    fill_idx, fill_val = _lines(600, T, V, 77)
    fill_idx[300:340], fill_val[300:340] = idx, val
    eng.encode(fill_idx, fill_val)
    inside = eng.decode_beam(batch_size=N, want_align=True, rejection_threshold=0.5)
    assert eng.stat('encoder_persistent') == 0
    _same([alone[k] for k in BEAM_KEYS], [inside[k][300:340] for k in BEAM_KEYS], 'never by batch')
    eng.close()


def test_handoffs_do_not_depend_on_timing():
    """Random small shapes on the persistent split encoder while a second stream of the process keeps the chip busy with GEMMs:
    every output equals the per-step form's and a repetition of itself."""
    import ctypes
    import threading
    from cor_asv_ann_amd.engine import HipEngine
    stop = []

    def background():                                 # a second handle = a second stream: 2048^3 contractions back to back
        e = HipEngine(1, 32, 16)
        ms = ctypes.c_double()
        while not stop:
            e.lib.casv_debug_gemm(e.handle, 0, 2048, 2048, 2048, 0, 20, ctypes.byref(ms))
        e.close()

    th = threading.Thread(target=background)
    th.start()
    try:
        rng = np.random.default_rng(11)
        for case in range(20):
            d = int(rng.integers(1, 5)); W = int(rng.choice([32, 64, 128, 256])); V = int(rng.choice([24, 64, 100]))
            B = int(rng.integers(1, 150)); T = int(rng.integers(2, 30))
            cfg = ModelConfig(depth=d, width=W, voc_size=V)
            eng = _engine(cfg, make_weights(cfg, seed=int(rng.integers(1, 1 << 30)), emb_scale=float(rng.choice([8., 24.]))))
            eng.set_option('arithmetic', 2)
            idx, val = _lines(B, T, V, int(rng.integers(1, 1 << 30)))
            step, s0, _ = _leg(eng, 0, idx, val, 4, search=False)
            for rep in range(2):
                pers, s1, _ = _leg(eng, 1, idx, val, 4, search=False)
                assert (s0, s1) == (0, 1)
                _same(step, pers, (case, rep, d, W, V, B, T))
            eng.close()
    finally:
        stop.append(1)
        th.join()


def test_two_handles_on_the_persistent_split_encoder_at_once():
    import threading
    cfg = ModelConfig(depth=2, width=128, voc_size=64)
    weights = make_weights(cfg, emb_scale=24.0)
    batches = [_lines(40 + 16 * k, 20 + k, 64, 900 + k) for k in range(4)]
    eng = _engine(cfg, weights)
    eng.set_option('arithmetic', 2)
    alone = [_leg(eng, 0, i, v, 4, search=False)[0] for i, v in batches]
    eng.close()
    errors = []

    def worker(order):
        try:
            e = _engine(cfg, weights)
            e.set_option('arithmetic', 2)
            for rep in range(5):
                for k in order:
                    got, st, _ = _leg(e, 1, batches[k][0], batches[k][1], 4, search=False)
                    if st != 1 or not all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, alone[k])):
                        errors.append((order, rep, k, st))
            e.close()
        except Exception as err:            # reported by the main thread
            errors.append(repr(err))

    threads = [threading.Thread(target=worker, args=(o,)) for o in ([0, 1, 2, 3], [3, 2, 1, 0])]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_give_up_path():
    """"persistent" = 3 (processes started with CASV_FAULT_INJECTION=1 only): one workgroup of the persistent split encoder
    leaves without handing on, its peers' bounded waits elapse, the launch returns with its give-up word set and the pass is
    redone per step -- same bits, statistic 0; the next 16 calls back off; the clean persistent call behind them resets the
    back-off.  One injected give-up, nothing is tried again."""
    assert os.environ.get('CASV_FAULT_INJECTION') == '1'
    cfg = ModelConfig(depth=2, width=64, voc_size=48)
    eng = _engine(cfg, make_weights(cfg, emb_scale=8.0))
    idx, val = _lines(21, 12, 48, 5)

    def search(p):
        eng.set_option('persistent', p)
        eng.encode(idx, val)
        res = eng.decode_beam(batch_size=4, want_align=True)
        return [res[k] for k in BEAM_KEYS], eng.stat('encoder_persistent')

    want, st = search(0)
    assert st == 0
    got, st = search(3)
    assert st == 0, 'a pass that gave up was redone per step'
    _same(want, got, 'give-up')
    for call in range(16):                            # the back-off: 16 calls leave the persistent form alone
        got, st = search(1)
        assert st == 0, call
        _same(want, got, 'behind the give-up')
    for call in range(2):                             # a clean persistent call, which resets the back-off: so is the next one
        got, st = search(1)
        assert st == 1, call
        _same(want, got, 'after the back-off')
    eng.close()
