"""Reproducible training: the train step's "deterministic" option (every sum in a fixed order), Adam's
state at the C ABI, and train(resume=...) through the facade."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import ModelConfig, make_weights, make_lines, vectorize_lines
from oracle.decode import OracleModel
from oracle.train import forward_backward

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _idx(a):
    return np.where(a.any(axis=2), a.argmax(axis=2), -1).astype(np.int32)


def _small_case(d, W, V, B, L, A=1, masks=True, flags=None, seed=4):
    """Weights, oracle inputs and the step's index arrays of a small batch (A > 1: confusion-network input, two alternatives)."""
    flags = flags or {}
    cfg = ModelConfig(depth=d, width=W, voc_size=V, **flags)
    w = make_weights(cfg, emb_scale=4.0)
    rng = np.random.default_rng(seed)
    for k in w:
        if k.endswith('_b') or k in ('att_bUW', 'att_bv'):
            w[k] = (w[k] + rng.normal(size=w[k].shape) * 0.2).astype(np.float32)
    om = OracleModel(cfg, w)
    src, sidx = make_lines(B, L, 1, voc_size=V)
    tgt, _ = make_lines(B, L, 2, voc_size=V)
    tgt[1] = tgt[1][:L // 2] + '\n'
    enc_in, dec_in, dec_out, wts = vectorize_lines(om, src, tgt)
    val = None
    if A > 1:
        alt = np.roll(sidx, 1, axis=1)
        sidx = np.stack([sidx, alt], axis=2).astype(np.int32)
        val = np.stack([np.full(alt.shape, 0.75), np.full(alt.shape, 0.25)], axis=2).astype(np.float32)
    C = cfg.ctx_width
    m = None
    if masks:
        keep = lambda shape: ((rng.random(shape) > 0.2) / 0.8).astype(np.float32)
        m = {'enc': [keep(2 * W if (n == 0 or cfg.deep_bidirectional_encoder) else W) for n in range(d)],
             'dec': [keep(W) for _ in range(d - 1)], 'cell': keep((B, W + C))}
    batch = (sidx, val, _idx(dec_in), _idx(dec_out), wts, m)
    return cfg, w, (enc_in, dec_in, dec_out, wts, m), batch


def _session(d, W, V, w, batch, steps, flags=None, options=None, frozen=()):
    """A fresh deterministic session: `steps` mode-1 steps, then the mode-2 gradients.  Everything the step leaves, as arrays."""
    from cor_asv_ann_amd.engine import HipEngine
    eng = HipEngine(d, W, V, **(flags or {}))
    try:
        eng.set_weights(w)
        eng.set_option('deterministic', 1)
        for k, v in (options or {}).items():
            eng.set_option(k, v)
        eng.train_begin(frozen=frozen)
        sidx, val, di, do, wts, m = batch
        out = {'loss': [], 'norm': []}
        for _ in range(steps):
            lo, no = eng.train_step(sidx, val, di, do, wts, m, mode=1)
            out['loss'].append(lo); out['norm'].append(no)
        out['eval'] = eng.train_step(sidx, val, di, do, wts, None, mode=0)[0]
        out['weights'] = eng.train_weights()
        out['m'], out['v'], out['step'] = eng.train_state()
        lo, no = eng.train_step(sidx, val, di, do, wts, m, mode=2)
        out['loss'].append(lo); out['norm'].append(no)
        out['grads'] = eng.train_gradients()
        eng.train_end()
        return out
    finally:
        eng.close()


def _assert_same_bits(a, b):
    assert a['loss'] == b['loss'] and a['norm'] == b['norm'] and a['eval'] == b['eval']
    assert a['step'] == b['step']
    for part in ('weights', 'm', 'v', 'grads'):
        assert set(a[part]) == set(b[part]), part
        for k in a[part]:
            assert np.array_equal(a[part][k], b[part][k]), (part, k)


def _c4_session(steps=3, options=None):
    from cor_asv_ann_amd.engine import HipEngine
    from tests.golden.make_c4_golden import DEPTH, WIDTH, VOC, c4_inputs
    cfg = ModelConfig(depth=DEPTH, width=WIDTH, voc_size=VOC)
    w = make_weights(cfg, emb_scale=4.0)
    sidx, dec_in, dec_out, wts, masks = c4_inputs()
    return _session(DEPTH, WIDTH, VOC, w, (sidx, None, dec_in, dec_out, wts, masks), steps, options=options)


def test_c4_deterministic_step_same_bits_twice_and_equals_oracle(golden_dir):
    """configs[3] at full size with dropout masks: two fresh sessions, three updates each, then the gradients -- every bit equal;
    and the deterministic step's gradients are still the oracle's (the fixture and tolerances of
    test_c4_full_size_step_equals_oracle)."""
    from cor_asv_ann_amd.engine import HipEngine
    from tests.golden.make_c4_golden import DEPTH, WIDTH, VOC, c4_inputs, sample_positions
    with np.load(os.path.join(golden_dir, 'c4_train_step.npz')) as f:
        g = {k: f[k] for k in f.files}
    cfg = ModelConfig(depth=DEPTH, width=WIDTH, voc_size=VOC)
    w = make_weights(cfg, emb_scale=4.0)
    sidx, dec_in, dec_out, wts, masks = c4_inputs()
    eng = HipEngine(DEPTH, WIDTH, VOC)
    eng.set_weights(w)
    eng.set_option('deterministic', 1)
    eng.train_begin()
    loss, norm = eng.train_step(sidx, None, dec_in, dec_out, wts, masks, mode=2)
    assert abs(loss - float(g['loss'])) < 2e-5 * abs(float(g['loss'])), (loss, float(g['loss']))
    assert abs(norm - float(g['grad_norm'])) < 1e-4 * float(g['grad_norm']), (norm, float(g['grad_norm']))
    onorm = float(g['grad_norm'])
    for k, got in eng.train_gradients().items():
        flat = got.ravel()
        scale = max(float(g['max/' + k]), 1e-6 * onorm)
        assert np.abs(flat[sample_positions(k, flat.size)] - g['sample/' + k]).max() < 2e-3 * scale + 1e-7, k
    assert eng.train_step(sidx, None, dec_in, dec_out, wts, masks, mode=2) == (loss, norm)
    eng.train_end()
    eng.close()
    _assert_same_bits(_c4_session(), _c4_session())


@pytest.mark.parametrize('case', ['plain', 'residual', 'bridge', 'deep', 'all', 'frozen', 'confusion', 'no_masks'])
def test_small_deterministic_step_same_bits_twice_and_equals_oracle(case):
    flags = {'residual': dict(residual_connections=True), 'bridge': dict(bridge_dense=True),
             'deep': dict(deep_bidirectional_encoder=True),
             'all': dict(deep_bidirectional_encoder=True, residual_connections=True, bridge_dense=True)}.get(case, {})
    d, W, V, B, L = (3, 64, 40, 6, 9) if case != 'plain' else (2, 96, 40, 5, 8)
    A = 2 if case == 'confusion' else 1
    cfg, w, (enc_in, dec_in, dec_out, wts, m), batch = _small_case(d, W, V, B, L, A=A, masks=case != 'no_masks', flags=flags)
    frozen = ('enc1_', 'dec1_') if case == 'frozen' else ()
    a = _session(d, W, V, w, batch, 3, flags=flags, frozen=frozen)
    b = _session(d, W, V, w, batch, 3, flags=flags, frozen=frozen)
    _assert_same_bits(a, b)
    if frozen:
        assert not any(k.startswith(frozen) for k in a['m'])
    if A == 1:
        # the first step's loss against the oracle (the tolerances of test_train_step_matches_oracle)
        from cor_asv_ann_amd.engine import HipEngine
        loss, grads, _ = forward_backward(cfg, w, enc_in, dec_in, dec_out, wts, m)
        onorm = np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in grads.values()))
        assert abs(a['loss'][0] - loss) < 2e-5 * abs(loss)
        if not frozen:
            assert abs(a['norm'][0] - onorm) < 1e-4 * onorm
        eng = HipEngine(d, W, V, **flags)
        eng.set_weights(w)
        eng.set_option('deterministic', 1)
        eng.train_begin()
        eng.train_step(*batch, mode=2)
        gg = eng.train_gradients()
        eng.train_end()
        eng.close()
        for k in grads:
            scale = max(np.abs(grads[k]).max(), 1e-6 * onorm)
            assert np.abs(gg[k] - grads[k]).max() < 2e-3 * scale + 1e-7, k


def test_deterministic_step_same_bits_whatever_the_launch_form():
    """persistent recurrences on / off, the fused backward step on / off: the deterministic step's bits do not move (at W 128 and
    B 37 the default step takes the persistent forms, and its bits differ between them)."""
    d, W, V, B, L = 3, 128, 40, 37, 7
    _, w, _, batch = _small_case(d, W, V, B, L)
    ref = _session(d, W, V, w, batch, 2)
    for opts in (dict(persistent=0), dict(persistent=1), dict(fused_backward=0), dict(persistent=0, fused_backward=0)):
        _assert_same_bits(ref, _session(d, W, V, w, batch, 2, options=opts))


# ------------------------------------------------------------------------------------------------------------------ earlier shapes
# A step's results do not depend on the shapes the session saw before: after a larger step every buffer of the session is larger
# than the target needs and holds older contents, after a smaller one every buffer must grow.
_HISTORY_MODELS = {'d2': (2, 32, 40, {}),
                   # (the most per-layer buffers: both directions' own outputs, the cross sums, the bridged states, the top sum)
                   'd3_all': (3, 64, 40, dict(deep_bidirectional_encoder=True, bridge_dense=True, residual_connections=True))}
_HISTORY_TARGET = (4, 7)                                    # B, L
_HISTORY_EARLIER = {'larger': (6, 12), 'smaller': (2, 3)}
_HISTORY_RUNS = {}


def _target_step(model, earlier, deterministic):
    """The target batch's mode-2 loss, norm and gradients, its mode-0 loss and the statistic "train_persistent_launches" of its mode-2
    step, in a session that ran `earlier` (None: nothing) first: one mode-2 step and one mode-0 step, which leave the weights alone.
    Computed once per process."""
    key = (model, earlier, deterministic)
    if key not in _HISTORY_RUNS:
        from cor_asv_ann_amd.engine import HipEngine
        d, W, V, flags = _HISTORY_MODELS[model]
        _, w, _, batch = _small_case(d, W, V, *_HISTORY_TARGET, flags=flags)
        eng = HipEngine(d, W, V, **flags)
        try:
            eng.set_weights(w)
            if deterministic:
                eng.set_option('deterministic', 1)
            eng.train_begin()
            if earlier:
                _, w0, _, b0 = _small_case(d, W, V, *_HISTORY_EARLIER[earlier], flags=flags)
                assert all(np.array_equal(w0[k], w[k]) for k in w)
                eng.train_step(*b0, mode=2)
                eng.train_step(*b0[:5], None, mode=0)
            out = dict(zip(('loss', 'norm'), eng.train_step(*batch, mode=2)))
            out['launches'] = eng.stat('train_persistent_launches')
            out['grads'] = eng.train_gradients()
            out['eval'] = eng.train_step(*batch[:5], None, mode=0)[0]
            eng.train_end()
        finally:
            eng.close()
        _HISTORY_RUNS[key] = out
    return _HISTORY_RUNS[key]


@pytest.mark.parametrize('earlier', sorted(_HISTORY_EARLIER))
@pytest.mark.parametrize('model', sorted(_HISTORY_MODELS))
def test_deterministic_step_same_bits_whatever_shapes_came_before(model, earlier):
    fresh, got = _target_step(model, None, True), _target_step(model, earlier, True)
    assert got['loss'] == fresh['loss'] and got['norm'] == fresh['norm'] and got['eval'] == fresh['eval']
    assert set(got['grads']) == set(fresh['grads'])
    for k in fresh['grads']:
        assert np.array_equal(got['grads'][k], fresh['grads'][k]), k


@pytest.mark.parametrize('earlier', sorted(_HISTORY_EARLIER))
def test_default_step_equals_oracle_whatever_shapes_came_before(earlier):
    """The default step (persistent recurrences where the shape has them, float atomics: no bits to compare): the gradients
    against the oracle (the tolerances of test_train_step_matches_oracle), and as many persistent launches as a fresh session takes."""
    d, W, V, flags = _HISTORY_MODELS['d2']
    cfg, w, (enc_in, dec_in, dec_out, wts, m), _ = _small_case(d, W, V, *_HISTORY_TARGET, flags=flags)
    if 'oracle' not in _HISTORY_RUNS:
        _HISTORY_RUNS['oracle'] = forward_backward(cfg, w, enc_in, dec_in, dec_out, wts, m)[1]
    grads = _HISTORY_RUNS['oracle']
    onorm = np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in grads.values()))
    fresh, got = _target_step('d2', None, False), _target_step('d2', earlier, False)
    assert got['launches'] == fresh['launches']
    for run in (fresh, got):
        for k in grads:
            scale = max(np.abs(grads[k]).max(), 1e-6 * onorm)
            assert np.abs(run['grads'][k] - grads[k]).max() < 2e-3 * scale + 1e-7, k


_CHILD = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_deterministic_train import _small_case, _session
_, w, _, batch = _small_case(3, 128, 40, 37, 7)
out = _session(3, 128, 40, w, batch, 2)
np.savez(sys.argv[2], loss=np.array(out['loss']), norm=np.array(out['norm']),
         **{'w/' + k: v for k, v in out['weights'].items()}, **{'g/' + k: v for k, v in out['grads'].items()})
'''


def test_deterministic_step_same_bits_under_attn_defer_variants(tmp_path):
    """CASV_ATTN_DEFER picks the persistent attention backward's form (read once per process): child processes with 0 and 3
    return the bits of this process's deterministic step."""
    _, w, _, batch = _small_case(3, 128, 40, 37, 7)
    ref = _session(3, 128, 40, w, batch, 2)
    for v in ('0', '3'):
        out = tmp_path / ('defer%s.npz' % v)
        env = dict(os.environ, CASV_ATTN_DEFER=v)
        subprocess.run([sys.executable, '-c', _CHILD, ROOT, str(out)], env=env, check=True, timeout=600)
        with np.load(out) as f:
            assert list(f['loss']) == ref['loss'] and list(f['norm']) == ref['norm']
            for k in ref['weights']:
                assert np.array_equal(f['w/' + k], ref['weights'][k]), k
            for k in ref['grads']:
                assert np.array_equal(f['g/' + k], ref['grads'][k]), k


def test_deterministic_step_same_bits_beside_another_training_handle():
    """A deterministic session whose steps run while a second handle trains (default options, persistent kernels that want every
    CU) on another thread returns the bits it returns alone."""
    from cor_asv_ann_amd.engine import HipEngine
    d, W, V, B, L = 2, 256, 48, 64, 12
    _, w, _, batch = _small_case(d, W, V, B, L)
    alone = _session(d, W, V, w, batch, 3)
    _, w2, _, batch2 = _small_case(2, 512, 64, 512, 16, masks=False, seed=7)
    other = HipEngine(2, 512, 64)
    other.set_weights(w2)
    other.train_begin()
    go, done = threading.Event(), threading.Event()

    def busy():
        go.wait()
        while not done.is_set():
            other.train_step(*batch2, mode=1)
    t = threading.Thread(target=busy)
    t.start()
    try:
        go.set()
        beside = _session(d, W, V, w, batch, 3)
    finally:
        done.set()
        t.join()
        other.train_end()
        other.close()
    _assert_same_bits(alone, beside)


def test_state_round_trip_continues_the_session():
    """Weights + Adam's moments + step count of a session after k steps, set into a fresh session: its next step is the first
    session's next step, bit for bit; without the state it is not."""
    from cor_asv_ann_amd.engine import HipEngine
    d, W, V, B, L = 2, 64, 40, 6, 9
    _, w, _, batch = _small_case(d, W, V, B, L)

    def fresh(weights):
        e = HipEngine(d, W, V)
        e.set_weights(weights)
        e.set_option('deterministic', 1)
        e.train_begin()
        return e
    a = fresh(w)
    for _ in range(3):
        a.train_step(*batch, mode=1)
    wk = a.train_weights()
    mk, vk, step = a.train_state()
    assert step == 3 and set(mk) == set(wk)
    la = a.train_step(*batch, mode=1)
    wa, (ma, va, sa) = a.train_weights(), a.train_state()
    b = fresh(wk)
    b.set_train_state(mk, vk, step)
    m2, v2, s2 = b.train_state()
    assert s2 == step and all(np.array_equal(m2[k], mk[k]) and np.array_equal(v2[k], vk[k]) for k in mk)
    lb = b.train_step(*batch, mode=1)
    wb, (mb, vb, sb) = b.train_weights(), b.train_state()
    assert la == lb and sa == sb == 4
    for k in wa:
        assert np.array_equal(wa[k], wb[k]) and np.array_equal(ma[k], mb[k]) and np.array_equal(va[k], vb[k]), k
    c = fresh(wk)                   # the weights alone: Adam starts over
    c.train_step(*batch, mode=1)
    wc = c.train_weights()
    assert any(not np.array_equal(wa[k], wc[k]) for k in wa)
    for e in (a, b, c):
        e.train_end()
        e.close()


def test_frozen_tensor_has_no_state():
    from cor_asv_ann_amd.engine import HipEngine
    from cor_asv_ann_amd._native import NativeError
    d, W, V = 2, 64, 40
    cfg = ModelConfig(depth=d, width=W, voc_size=V)
    eng = HipEngine(d, W, V)
    eng.set_weights(make_weights(cfg, emb_scale=4.0))
    eng.train_begin(frozen=('enc1_',))
    a = np.zeros(eng.pshapes['enc1_fw_K'], np.float32)
    with pytest.raises(NativeError, match='frozen'):
        import cor_asv_ann_amd._native as nv
        nv.check(eng.lib.casv_train_get_state(eng.handle, b'enc1_fw_K', 0, nv.ptr(a), a.size))
    m, v, step = eng.train_state()
    assert 'enc1_fw_K' not in m and 'enc2_K' in m and step == 0
    eng.train_end()
    eng.close()


def _copy_task(tmp_path):
    rng = np.random.default_rng(0)
    alphabet = 'abcdefgh '
    lines = [''.join(rng.choice(list(alphabet), size=rng.integers(4, 10))) for _ in range(240)]
    (tmp_path / 'train.tsv').write_text(''.join('%s\t%s\n' % (l, l) for l in lines))
    return str(tmp_path / 'train.tsv')


def _model(epochs, state=True):
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence
    s2s = Sequence2Sequence(progbars=False)
    s2s.depth, s2s.width, s2s.batch_size, s2s.epochs = 2, 32, 32, epochs
    s2s.seed, s2s.deterministic, s2s.checkpoint_training_state = 11, True, state
    return s2s


def test_facade_resume_equals_an_uninterrupted_run(tmp_path, monkeypatch):
    import glob
    monkeypatch.chdir(tmp_path)
    corpus = _copy_task(tmp_path)
    (tmp_path / 'full').mkdir(); (tmp_path / 'cut').mkdir(); (tmp_path / 'plain').mkdir()
    monkeypatch.chdir(tmp_path / 'full')
    full = _model(4)
    full.configure()
    full.train([corpus])
    monkeypatch.chdir(tmp_path / 'cut')
    first = _model(2)
    first.configure()
    first.train([corpus])
    ckpt = sorted(glob.glob('model.ckpt.weights-02-*.h5'))
    assert len(ckpt) == 1
    resumed = _model(4)
    resumed.configure()
    resumed.train([corpus], resume=ckpt[0])
    assert resumed.history == full.history and resumed.status == full.status == 2
    for k, v in full._weights.items():
        assert np.array_equal(resumed._weights[k], v), k
    # the weights of the checkpoint alone (Adam, generator and EarlyStopping start over) give another run
    monkeypatch.chdir(tmp_path / 'plain')
    plain = _model(2)
    plain.load_config(os.path.join(str(tmp_path / 'cut'), ckpt[0]))
    plain.configure()
    plain.load_weights(os.path.join(str(tmp_path / 'cut'), ckpt[0]))
    plain.status = 1
    plain.train([corpus])
    assert any(not np.array_equal(plain._weights[k], v) for k, v in full._weights.items())
