"""Layer 1 of the search's per-step encoder from the per-character table (csrc/encoder.hip, option "encoder_table"), and the search's
last iteration without its decoder step (csrc/decode.hip, option "beam_skip_last"), on a real MI355X.

Both changes remove work the result does not need, so every comparison here is of the bits: the table hands a cell the
accumulators its own x columns would have left (tests/test_gpu_acc_in.py holds that at the GEMM), and nothing reads what the
decoder step of iteration S - 1 writes.  The statistics "encoder_table" (the last encoder pass read the table) and
"encoder_ahead" (it took the upper layers' input terms ahead, option value 2) and "encoder_table_builds" (tables built on the handle)
say which path ran.  Runs that are compared use a handle each: none finds the other's results in its buffers.
"""
import numpy as np
import pytest

from oracle import ModelConfig, make_weights

pytestmark = pytest.mark.gpu

V = 64
BEAM_KEYS = ('idx', 'len', 'n_found', 'n_steps', 'score', 'prob', 'rej')


def _engine(cfg, weights, arithmetic=2):
    from cor_asv_ann_amd.engine import HipEngine
    eng = HipEngine(cfg.depth, cfg.width, cfg.voc_size)
    eng.set_weights(weights)
    eng.set_option('arithmetic', arithmetic)
    return eng


def _lines(B, T, seed):
    """plain-text lines of unequal length (-1 behind a line's end), line 5 empty, line 6 full"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, V, (B, T)).astype(np.int32)
    lens = rng.integers(0, T + 1, B)
    lens[5], lens[6] = 0, T
    idx[np.arange(T)[None, :] >= lens[:, None]] = -1
    return idx


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _encoded(eng, idx, val=None):
    eng.encode(idx, val)
    enc, states = eng.encoder_outputs()
    return enc, np.stack(states), eng.stat('encoder_table'), eng.stat('encoder_persistent')


@pytest.mark.parametrize('depth', [2, 4])
def test_encoder_outputs_states_and_u_with_the_option_0_1_2(depth):
    """257 and 300 lines (per-step form), T = 1 and 7, both split arithmetics: outputs, final states and u of option 1 (layer 1 from the
    table) and 2 (and the upper layers' input terms ahead) are option 0's.  One handle per option, so that no run finds another's
    results in its buffers."""
    cfg = ModelConfig(depth=depth, width=128, voc_size=V)
    weights = make_weights(cfg, emb_scale=16.0)
    for arithmetic in (1, 2):
        engs = {}
        for opt in (2, 1, 0):
            engs[opt] = _engine(cfg, weights, arithmetic)
            engs[opt].set_option('encoder_table', opt)
        for B in (257, 300):
            for T in (1, 7):
                idx = _lines(B, T, 100 * B + T)
                got = {}
                for opt in (2, 1, 0):
                    enc, st, used, persistent = _encoded(engs[opt], idx)
                    assert (used, engs[opt].stat('encoder_ahead'), persistent) == (int(opt >= 1), int(opt == 2), 0), (opt, B, T)
                    got[opt] = (enc, st, engs[opt].debug_u())
                    assert np.isfinite(enc).all()
                for opt in (1, 2):
                    for name, a, b in zip(('enc', 'states', 'u'), got[0], got[opt]):
                        assert _same_bits(a, b), (arithmetic, opt, B, T, name)
        for opt in (1, 2):
            assert engs[opt].stat('encoder_table_builds') == 1         # one table per commit, whatever the batches
        for eng in engs.values():
            eng.close()


def test_search_results_do_not_depend_on_the_batch_or_the_option():
    """The same 300 lines searched in one call (per-step encoder) with the option 1, 2 and 0 -- a handle each -- and in calls of <= 256
    lines (another launch form): every line's result is the same bits."""
    cfg = ModelConfig(depth=2, width=128, voc_size=V)
    weights = make_weights(cfg, emb_scale=16.0)
    idx = _lines(300, 7, 7)
    res = {}
    for opt in (1, 2, 0):
        eng = _engine(cfg, weights, arithmetic=-1)
        eng.set_option('encoder_table', opt)
        eng.encode(idx)
        res[opt] = eng.decode_beam(batch_size=8)
        assert (eng.stat('encoder_table'), eng.stat('encoder_ahead')) == (int(opt >= 1), int(opt == 2)), opt
        eng.close()
    for opt in (1, 2):
        for k in BEAM_KEYS:
            assert np.array_equal(res[0][k], res[opt][k], equal_nan=True), (opt, k)
    eng = _engine(cfg, weights, arithmetic=-1)
    for lo, hi in ((0, 256), (256, 300)):
        eng.encode(idx[lo:hi])
        part = eng.decode_beam(batch_size=8)
        for k in BEAM_KEYS:
            assert np.array_equal(res[1][k][lo:hi], part[k], equal_nan=True), (k, lo, hi)
    eng.close()


def test_confusion_networks_and_the_chain_arithmetic_keep_the_old_path():
    cfg = ModelConfig(depth=2, width=128, voc_size=V)
    weights = make_weights(cfg, emb_scale=16.0)
    eng = _engine(cfg, weights, 2)
    idx = _lines(300, 7, 11)
    # two alternatives per position
    idx2 = np.stack([idx, np.where(idx >= 0, (idx + 1) % V, -1)], axis=2).astype(np.int32)
    val2 = np.where(idx2 >= 0, np.float32(0.5), np.float32(0)).astype(np.float32)
    assert _encoded(eng, idx2, val2)[2] == 0
    # one alternative, but a weight that is not 1
    val1 = np.where(idx >= 0, np.float32(0.75), np.float32(0)).astype(np.float32)[:, :, None]
    assert _encoded(eng, idx, val1)[2] == 0
    assert _encoded(eng, idx)[2] == 1
    eng.close()
    chain = _engine(cfg, weights, 0)
    assert _encoded(chain, idx)[2] == 0
    assert chain.stat('encoder_table_builds') == 0
    chain.close()


def test_new_weights_get_a_new_table():
    cfg = ModelConfig(depth=2, width=128, voc_size=V)
    w1, w2 = make_weights(cfg, emb_scale=16.0), make_weights(cfg, emb_scale=8.0)
    idx = _lines(257, 7, 3)
    eng = _engine(cfg, w1, 2)
    enc1, st1, used, _ = _encoded(eng, idx)
    assert used == 1 and eng.stat('encoder_table_builds') == 1
    eng.set_weights(w2)
    enc2, st2, used, _ = _encoded(eng, idx)
    assert used == 1 and eng.stat('encoder_table_builds') == 2
    fresh = _engine(cfg, w2, 2)
    enc3, st3, used, _ = _encoded(fresh, idx)
    assert used == 1
    assert _same_bits(enc2, enc3) and _same_bits(st2, st3)
    assert not _same_bits(enc1, enc2)
    eng.close(); fresh.close()


@pytest.mark.parametrize('lm', [0, 1])
@pytest.mark.parametrize('N', [1, 8])
def test_the_last_iteration_without_its_decoder_step_changes_nothing(N, lm):
    """Searches of S = 1, 2, 5 iterations on 3 lines: every returned array, n_steps and both kinds of alignments equal what the same
    build returns with the step launched (option "beam_skip_last" = 0)."""
    cfg = ModelConfig(depth=2, width=128, voc_size=V)
    weights = make_weights(cfg, emb_scale=16.0)
    idx = _lines(8, 4, 21)[5:8]             # an empty line, a full one, one more
    other = _lines(8, 4, 22)[5:8]
    engs = {}
    for skip in (1, 0):
        engs[skip] = _engine(cfg, weights, arithmetic=-1)
        engs[skip].set_option('lm_predict', lm)
        engs[skip].set_option('beam_skip_last', skip)
    for S in (1, 2, 5):
        for align in (True, 'sparse'):
            out = {}
            for skip in (1, 0):
                # a longer search of OTHER lines first: slot S of every store then holds data of theirs -- whoever read it would show
                engs[skip].encode(other)
                engs[skip].decode_beam(batch_size=N, steps=8)
                engs[skip].encode(idx)
                out[skip] = engs[skip].decode_beam(batch_size=N, steps=S, want_align=align)
            for k in BEAM_KEYS + (('align',) if align is True else ()):
                assert np.array_equal(out[0][k], out[1][k], equal_nan=True), (S, align, k)
            if align == 'sparse':
                for a, b in zip(out[0]['align_sparse'], out[1]['align_sparse']):
                    assert np.array_equal(a, b, equal_nan=True), (S, 'align_sparse')
            assert (out[1]['n_steps'] <= S).all()
    for eng in engs.values():
        eng.close()
