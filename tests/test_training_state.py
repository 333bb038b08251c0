"""Resumable training on the host side: the training-state group of the checkpoint container (keras_h5), the generator state,
and train()'s checkpoint / resume bookkeeping against a stand-in engine (the device step is tested in
tests/test_gpu_deterministic_train.py)."""
import os
import signal
import subprocess

import numpy as np
import pytest

from cor_asv_ann_amd import keras_h5
from cor_asv_ann_amd.seq2seq import Sequence2Sequence
from oracle.weights import ModelConfig, make_vocabulary, make_weights

from tests.test_hdf5 import H5PY_PYTHON


def _model(d=2, W=16, V=12):
    s2s = Sequence2Sequence(progbars=False)
    s2s.depth, s2s.width, s2s.voc_size = d, W, V
    s2s.mapping = make_vocabulary(V)
    s2s.configure()
    return s2s


def _state(weights, rng):
    return {'epoch': 3, 'step': 41, 'wait': 1, 'best_epoch': 2, 'best_val_loss': 0.123456789012345, 'adam': [1e-3, 0.9, 0.999, 1e-7, 5.0],
            'frozen': ['enc1_', 'dec1_'], 'rng': rng.bit_generator.state, 'split_rand': rng.uniform(0, 1, 17),
            'history': [{'loss': 1.5, 'val_loss': 0.2}, {'loss': 1.25, 'val_loss': 0.123456789012345}, {'loss': 1.0, 'val_loss': 0.3}],
            'm': {k: (v * 0.5).astype(np.float32) for k, v in weights.items() if not k.startswith(('enc1_', 'dec1_'))},
            'v': {k: (v * v).astype(np.float32) for k, v in weights.items() if not k.startswith(('enc1_', 'dec1_'))},
            'best': {k: (v + 1).astype(np.float32) for k, v in weights.items()}}


def test_container_round_trip_is_exact(tmp_path):
    s2s = _model()
    w = make_weights(ModelConfig(depth=2, width=16, voc_size=12))
    st = _state(w, np.random.default_rng(5))
    path = str(tmp_path / 'ckpt.h5')
    keras_h5.write_model(path, s2s._config_dict(), w, st)
    got = keras_h5.read_training_state(path)
    assert set(got) == set(st)
    for key in ('epoch', 'step', 'wait', 'best_epoch', 'best_val_loss', 'adam', 'frozen', 'rng', 'history'):
        assert got[key] == st[key], key
    assert np.array_equal(got['split_rand'], st['split_rand'])
    for sub in ('m', 'v', 'best'):
        assert set(got[sub]) == set(st[sub])
        for k in st[sub]:
            assert got[sub][k].dtype == np.float32 and np.array_equal(got[sub][k], st[sub][k]), (sub, k)


def test_no_split_and_no_history_round_trip(tmp_path):
    s2s = _model()
    w = make_weights(ModelConfig(depth=2, width=16, voc_size=12))
    st = dict(_state(w, np.random.default_rng(5)), split_rand=None, history=[], frozen=[], best={}, best_epoch=0, best_val_loss=np.inf)
    path = str(tmp_path / 'ckpt.h5')
    keras_h5.write_model(path, s2s._config_dict(), w, st)
    got = keras_h5.read_training_state(path)
    assert got['split_rand'] is None and got['history'] == [] and got['frozen'] == [] and got['best'] == {}
    assert got['best_val_loss'] == np.inf


def test_rng_state_round_trip(tmp_path):
    """The generator continues after a trip through the file exactly as it would have."""
    s2s = _model()
    rng = np.random.default_rng(1234)
    rng.uniform(0, 1, 1001)
    w = make_weights(ModelConfig(depth=2, width=16, voc_size=12))
    path = str(tmp_path / 'ckpt.h5')
    st = dict(_state(w, np.random.default_rng(5)), rng=rng.bit_generator.state)
    keras_h5.write_model(path, s2s._config_dict(), w, st)
    again = np.random.default_rng()
    again.bit_generator.state = keras_h5.read_training_state(path)['rng']
    assert np.array_equal(again.uniform(0, 1, 64), rng.uniform(0, 1, 64))
    assert np.array_equal(again.integers(0, 1 << 62, 8), rng.integers(0, 1 << 62, 8))


def test_seed_makes_configure_repeatable():
    a, b = Sequence2Sequence(), Sequence2Sequence()
    for s in (a, b):
        s.depth, s.width, s.voc_size, s.seed = 2, 16, 12, 7
        s.configure()
    for k in a._weights:
        assert np.array_equal(a._weights[k], b._weights[k]), k
    c = Sequence2Sequence()
    c.depth, c.width, c.voc_size = 2, 16, 12
    assert c.seed is None and c.deterministic is False and c.checkpoint_training_state is False
    c.configure()
    assert any(not np.array_equal(a._weights[k], c._weights[k]) for k in a._weights)


CHECK_WITH_H5PY = r'''
import sys, h5py, numpy as np
with h5py.File(sys.argv[1], 'r') as f:
    names = [n.decode() for n in f.attrs['layer_names']]
    assert 'training_state' not in names
    out = {}
    for lname in names:
        g = f[lname]
        for wn in g.attrs['weight_names']:
            out[lname + '|' + wn.decode()] = g[wn.decode()][()]
    s = f['training_state']
    out['step'] = s['step'][()]
    out['m_E'] = s['m']['E'][()]
    out['rng'] = np.frombuffer(s['rng'][()], np.uint8)
np.savez(sys.argv[2], **out)
'''


def test_state_file_loads_as_plain_weights(tmp_path):
    """A checkpoint with the state group loads through load_weights and load_transfer_weights like any other."""
    s2s = _model()
    w = make_weights(ModelConfig(depth=2, width=16, voc_size=12))
    st = _state(w, np.random.default_rng(5))
    path = str(tmp_path / 'ckpt.h5')
    keras_h5.write_model(path, s2s._config_dict(), w, st)
    other = _model()
    other.load_weights(path)
    for k, v in w.items():
        assert np.array_equal(other.get_weights()[k], v), k
    deeper = _model(d=3)
    deeper.load_transfer_weights(path)
    assert np.array_equal(deeper.get_weights()['E'], w['E'])


def test_state_file_reads_with_libhdf5(tmp_path):
    """libhdf5 reads a state-carrying checkpoint: the layers in keras' loading order, the state group beside them (through the
    interpreter with h5py that tests/test_hdf5.py uses, where the machine has one)."""
    from tests.test_hdf5 import _h5py_available
    s2s = _model()
    w = make_weights(ModelConfig(depth=2, width=16, voc_size=12))
    st = _state(w, np.random.default_rng(5))
    path = str(tmp_path / 'ckpt.h5')
    keras_h5.write_model(path, s2s._config_dict(), w, st)
    if not _h5py_available():
        pytest.skip('no interpreter with h5py on this machine')
    script = tmp_path / 'check.py'
    script.write_text(CHECK_WITH_H5PY)
    dump = str(tmp_path / 'dump.npz')
    subprocess.run([H5PY_PYTHON, str(script), path, dump], check=True, timeout=300)
    with np.load(dump) as got:
        assert int(got['step']) == 41 and np.array_equal(got['m_E'], st['m']['E'])
        assert bytes(got['rng']).decode().startswith('{')
        table, knames = keras_h5.layer_tensors(2), keras_h5._keras_weight_names(2)
        for lname, tensors in table.items():
            for t, kn in zip(tensors, knames[lname]):
                assert np.array_equal(got[lname + '|' + kn].reshape(w[t].shape), w[t]), t


class _FakeEngine(object):
    """What train() asks of HipEngine, on the host: a 'step' moves every weight by a constant."""

    def __init__(self, s2s, interrupt_at=None, val_rises=False):
        from cor_asv_ann_amd.engine import weight_shapes
        self.interrupt_at, self.val_rises = interrupt_at, val_rises
        self.pshapes = weight_shapes(s2s.depth, s2s.width, s2s.voc_size)
        self.w = {k: np.array(v) for k, v in s2s._weights.items()}
        self.step, self.options, self.begun = 0, {}, None

    def set_option(self, key, value):
        self.options[key] = value

    def train_begin(self, *adam, frozen=()):
        self.begun = (adam, frozen)

    def set_train_state(self, m, v, step):
        self.step = step

    def train_step(self, idx, val, dec_in, dec_out, w, masks=None, mode=1):
        if mode == 1:
            self.step += 1
            for k in self.w:
                self.w[k] = self.w[k] + np.float32(0.01)
            if self.step == self.interrupt_at:          # a SIGINT arrives while this batch trains (StopSignalCallback)
                os.kill(os.getpid(), signal.SIGINT)
        if mode == 0 and self.val_rises:
            return float(self.step), 0.0
        return 1.0 / (1 + self.step), 0.0

    def train_weights(self):
        return {k: np.array(v) for k, v in self.w.items()}

    def train_state(self):
        return {k: np.zeros_like(v) for k, v in self.w.items()}, {k: np.ones_like(v) for k, v in self.w.items()}, self.step

    def get_weights(self):
        return self.train_weights()

    def train_end(self):
        pass


def _train(tmp_path, monkeypatch, epochs, state, resume=None, mutate=None, **fake):
    rng = np.random.default_rng(0)
    lines = [''.join(rng.choice(list('abcdef '), size=rng.integers(3, 8))) for _ in range(400)]
    corpus = tmp_path / 'train.tsv'
    corpus.write_text(''.join('%s\t%s\n' % (l, l) for l in lines))
    s2s = Sequence2Sequence(progbars=False)
    s2s.depth, s2s.width, s2s.batch_size, s2s.epochs, s2s.seed, s2s.checkpoint_training_state = 1, 16, 16, epochs, 3, state
    s2s.configure()
    if mutate:
        mutate(s2s)
    eng = {}
    monkeypatch.setattr(s2s, '_require_engine', lambda: eng.setdefault('e', _FakeEngine(s2s, **fake)))
    s2s.train([str(corpus)], resume=resume)
    return s2s, eng['e']


def test_checkpoints_carry_state_only_when_asked(tmp_path, monkeypatch):
    import glob
    monkeypatch.chdir(tmp_path)
    _train(tmp_path, monkeypatch, 1, False)
    (ck,) = glob.glob('model.ckpt.weights-01-*.h5')
    assert keras_h5.read_training_state(ck) is None
    with pytest.raises(ValueError, match='weights only'):
        _train(tmp_path, monkeypatch, 2, True, resume=ck)
    os.remove(ck)
    s2s, eng = _train(tmp_path, monkeypatch, 2, True)
    assert eng.options['deterministic'] == 0
    (ck,) = glob.glob('model.ckpt.weights-01-*.h5')
    st = keras_h5.read_training_state(ck)
    assert st['epoch'] == 1 and st['step'] == eng.step // 2 and len(st['history']) == 1 and st["split_rand"].shape == (400,)
    # resumed from epoch 1: the second epoch again, on the generator, split, history and step the file holds
    resumed, eng2 = _train(tmp_path, monkeypatch, 2, True, resume=ck)
    assert resumed.history == s2s.history and eng2.step == eng.step
    for k, v in s2s._weights.items():
        assert np.array_equal(resumed._weights[k], v), k


@pytest.mark.parametrize('mutate,what', [(lambda s: setattr(s, 'frozen_prefixes', ['enc1_']), 'frozen'),
                                         (lambda s: setattr(s, 'residual_connections', True), 'residual_connections')])
def test_mismatched_resume_is_refused(tmp_path, monkeypatch, mutate, what):
    import glob
    monkeypatch.chdir(tmp_path)
    _train(tmp_path, monkeypatch, 1, True)
    (ck,) = glob.glob('model.ckpt.weights-01-*.h5')
    with pytest.raises(ValueError, match=what):
        _train(tmp_path, monkeypatch, 2, True, resume=ck, mutate=mutate)


def test_mismatched_width_is_refused(tmp_path, monkeypatch):
    import glob
    monkeypatch.chdir(tmp_path)
    _train(tmp_path, monkeypatch, 1, True)
    (ck,) = glob.glob('model.ckpt.weights-01-*.h5')

    def wider(s):
        s.width = 32
        s.configure()
    with pytest.raises(ValueError, match='width'):
        _train(tmp_path, monkeypatch, 2, True, resume=ck, mutate=wider)


def test_epoch_cut_short_by_sigint_carries_no_state(tmp_path, monkeypatch):
    """A SIGINT inside epoch 2 ends the run after that epoch's validation; its checkpoint holds the weights only (the epoch is not
    complete, the generator has drawn part of it), so the run resumes from epoch 1's checkpoint and trains epoch 2 again -- ending
    where a run that was never stopped ends."""
    import glob
    for sub in ('full', 'cut'):
        (tmp_path / sub).mkdir()
    monkeypatch.chdir(tmp_path / 'full')
    full, feng = _train(tmp_path, monkeypatch, 3, True)
    per_epoch = feng.step // 3
    monkeypatch.chdir(tmp_path / 'cut')
    cut, ceng = _train(tmp_path, monkeypatch, 3, True, interrupt_at=per_epoch + 2)
    assert len(cut.history) == 2 and ceng.step == per_epoch + 2
    (ck2,) = glob.glob('model.ckpt.weights-02-*.h5')
    assert keras_h5.read_training_state(ck2) is None
    with pytest.raises(ValueError, match='weights only'):
        _train(tmp_path, monkeypatch, 3, True, resume=ck2)
    (ck1,) = glob.glob('model.ckpt.weights-01-*.h5')
    resumed, reng = _train(tmp_path, monkeypatch, 3, True, resume=ck1)
    assert resumed.history == full.history and reng.step == feng.step
    for k, v in full._weights.items():
        assert np.array_equal(resumed._weights[k], v), k


def test_resume_after_early_stopping_trains_no_further(tmp_path, monkeypatch):
    """val_loss rises after epoch 1: EarlyStopping(patience=3) ends the run after epoch 4.  Resumed from that checkpoint with more
    epochs asked for, the run ends there too, with the best epoch's weights."""
    import glob
    monkeypatch.chdir(tmp_path)
    full, feng = _train(tmp_path, monkeypatch, 6, True, val_rises=True)
    assert len(full.history) == 4
    (ck4,) = glob.glob('model.ckpt.weights-04-*.h5')
    assert keras_h5.read_training_state(ck4)['wait'] == 3
    resumed, reng = _train(tmp_path, monkeypatch, 6, True, resume=ck4, val_rises=True)
    assert resumed.history == full.history and reng.step == feng.step and resumed.status == full.status == 2
    for k, v in full._weights.items():
        assert np.array_equal(resumed._weights[k], v), k
