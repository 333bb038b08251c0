"""CPU checks of the soft-target feature: the float64 head of tests/soft_target_cases.py is the definition (torch autograd), the
noise bound catches every wrong head, alternatives_to_soft_targets builds the lists, train()'s distillation checks raise."""
import glob
import os

import numpy as np
import pytest

from cor_asv_ann_amd import keras_h5
from cor_asv_ann_amd.seq2seq import Sequence2Sequence, alternatives_to_soft_targets
from tests import soft_target_cases as sc

SMALL = [c for c in sc.HEAD_CASES if c[2] <= 5]


def _slot_probabilities(x, idx):
    p = np.exp(x.astype(np.float64) - x.astype(np.float64).max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    return np.take_along_axis(p, np.where(idx >= 0, idx, 0), axis=1)[idx >= 0]


@pytest.mark.parametrize('case', sc.HEAD_CASES, ids=lambda c: 'V%d_K%d_R%d' % c)
def test_rows_keep_clear_of_the_clip_edges(case):
    """No slot's probability is within 1e-3 (relative) of a clip edge: float32 and float64 agree on every ok_k."""
    (x, idx, q, w, inv_count, kinds), _, _ = sc.reference(case)
    pk = _slot_probabilities(x, idx)
    assert np.abs(pk / float(sc.LO) - 1.0).min(initial=1.0) > 1e-3
    assert np.abs((1.0 - pk) / (1.0 - float(sc.HI)) - 1.0).min(initial=1.0) > 1e-3       # (the upper edge: by the distance from 1)
    assert len({tuple(sorted(r[r >= 0])) for r in idx}) >= 1 and all(len(set(r[r >= 0])) == (r >= 0).sum() for r in idx)


def test_every_row_kind_appears_in_the_small_cases_and_clipped_entries_exist():
    seen = set()
    for case in SMALL:
        seen.update(sc.reference(case)[0][5])
    assert seen == set(sc.ROW_KINDS)
    (x, idx, q, w, inv_count, kinds), _, _ = sc.reference((96, 3, 8197))
    pk = _slot_probabilities(x, idx)
    assert (pk < 1e-7).any() and (pk > 1 - 1e-7).any()


@pytest.mark.parametrize('case', SMALL + [(65, 64, 8197)], ids=lambda c: 'V%d_K%d_R%d' % c)
def test_float64_head_is_autograd_of_the_clipped_cross_entropy(case):
    """-(q * log(clamp(softmax(x), 1e-7, 1 - 1e-7))).sum() x w x inv_count, differentiated by torch in float64: the definition's
    loss and dlogits to 1e-12 relative (test_rows_keep_clear_of_the_clip_edges: no probability within 1e-9 of an edge)."""
    import torch
    (x, idx, q, w, inv_count, _), (loss, d), _ = sc.reference(case)
    R, V = x.shape
    y = np.zeros((R, V), np.float64)
    for r in range(R):
        live = idx[r] >= 0
        y[r, idx[r][live]] = q[r][live].astype(np.float64)
    xt = torch.tensor(x.astype(np.float64), requires_grad=True)
    p = torch.softmax(xt, dim=1)
    ce = -(torch.tensor(y) * torch.log(torch.clamp(p, float(sc.LO), float(sc.HI)))).sum(dim=1)
    total = (ce * torch.tensor(w.astype(np.float64)) * float(inv_count)).sum()
    total.backward()
    assert abs(float(total) - loss) <= 1e-12 * max(abs(loss), 1e-30)
    g = xt.grad.numpy()
    assert np.abs(g - d).max() <= 1e-12 * max(np.abs(d).max(), 1e-30)


def test_every_wrong_head_is_caught():
    """Each wrong head misses the float64 head by at least 4 x the bound (C x the noise unit) on at least one case."""
    worst = {name: 0.0 for name in sc.WRONG_HEADS}
    for case in sc.HEAD_CASES:
        (x, idx, q, w, inv_count, _), f64, f32 = sc.reference(case)
        bound = sc.bounds(f32, f64)
        V = case[0]
        for name in sc.WRONG_HEADS:
            bad = sc.head(x, idx, q, w, inv_count, np.float64, wrong=name, pad=((V + 31) & ~31) - V)
            worst[name] = max(worst[name], max(e / b for e, b in zip(sc.errors(bad, f64), bound)))
    assert len(sc.WRONG_HEADS) >= 6
    for name, ratio in worst.items():
        assert ratio >= 4.0, (name, ratio)


def test_the_float32_head_is_within_its_own_unit_and_the_constant_is_twice_the_measurement():
    for case in SMALL:
        _, f64, f32 = sc.reference(case)
        assert all(e <= b for e, b in zip(sc.errors(f32, f64), sc.bounds(f32, f64, c=1.0)))
    assert sc.MEASURED_MAX_RATIO is not None and 2.0 * sc.MEASURED_MAX_RATIO <= sc.C < 2.0 * sc.MEASURED_MAX_RATIO + 1.0


# ---- alternatives_to_soft_targets ----
def _lists():
    alt_idx = np.array([[[3, 1, 2], [4, 0, 1], [2, 3, 4], [-1, -1, -1]],
                        [[1, 2, 3], [0, 1, 2], [5, 4, 3], [1, 2, 3]]], np.int32)
    alt_logp = np.log(np.array([[[0.5, 0.3, 0.1], [0.6, 0.2, 0.1], [0.4, 0.3, 0.2], [np.nan] * 3],
                                [[0.7, 0.2, 0.05], [0.5, 0.25, 0.125], [0.9, 0.05, 0.01], [0.3, 0.3, 0.3]]])).astype(np.float32)
    dec_out = np.array([[1, 5, -1, 2], [1, 2, 0, -1]], np.int32)       # inside, outside, unscored, invalid teacher row | ...
    return alt_idx, alt_logp, dec_out


def test_alpha_one_gives_the_one_hot_lists():
    alt_idx, alt_logp, dec_out = _lists()
    si, sq = alternatives_to_soft_targets(alt_idx, alt_logp, dec_out, alpha=1.0)
    assert si.shape == sq.shape == (2, 4, 4) and si.dtype == np.int32 and sq.dtype == np.float32
    scored = dec_out >= 0
    assert np.array_equal(si[..., 0], dec_out) and np.all(si[..., 1:] == -1)
    assert np.array_equal(sq[..., 0], scored.astype(np.float32)) and np.all(sq[..., 1:] == 0)


@pytest.mark.parametrize('renormalise', [True, False])
def test_soft_lists_hold_teacher_and_target_mass(renormalise):
    alt_idx, alt_logp, dec_out = _lists()
    alpha = 0.25
    si, sq = alternatives_to_soft_targets(alt_idx, alt_logp, dec_out, alpha=alpha, renormalise=renormalise)
    p = np.exp(alt_logp.astype(np.float64))
    for b in range(2):
        for u in range(4):
            t = dec_out[b, u]
            if t < 0:                                            # unscored: all slots empty
                assert np.all(si[b, u] == -1)
                continue
            if alt_idx[b, u, 0] < 0:                             # invalid teacher row: the one-hot row
                assert si[b, u].tolist() == [t, -1, -1, -1] and sq[b, u, 0] == 1.0
                continue
            mass = p[b, u] / p[b, u].sum() if renormalise else p[b, u]
            want = {int(v): (1 - alpha) * m for v, m in zip(alt_idx[b, u], mass)}
            inside = t in want
            want[int(t)] = want.get(int(t), 0.0) + alpha
            live = si[b, u] >= 0
            assert len(set(si[b, u][live])) == live.sum() == (3 if inside else 4)
            assert (si[b, u, 3] == -1) == inside                 # the spare slot is used only for a target outside the K
            got = dict(zip(si[b, u][live].tolist(), sq[b, u][live].tolist()))
            assert set(got) == set(want)
            for v in want:
                assert abs(got[v] - want[v]) < 1e-6
            if renormalise:
                assert abs(sq[b, u][live].sum() - 1.0) < 1e-6
    assert np.all(np.isfinite(sq)) and np.all(sq >= 0)


def test_soft_lists_refuse_bad_arguments():
    alt_idx, alt_logp, dec_out = _lists()
    with pytest.raises(ValueError, match='alpha'):
        alternatives_to_soft_targets(alt_idx, alt_logp, dec_out, alpha=1.5)
    with pytest.raises(ValueError, match='rows,U'):
        alternatives_to_soft_targets(alt_idx, alt_logp, dec_out[:, :3])


# ---- train(teacher=...): the checks, with a stub engine ----
class _StubEngine(object):
    """What train() asks of HipEngine on the host; a soft step counts as a step, the teacher's lists are the first K indices."""

    def __init__(self, s2s):
        from cor_asv_ann_amd.engine import weight_shapes
        self.pshapes = weight_shapes(s2s.depth, s2s.width, s2s.voc_size)
        self.w = {k: np.array(v) for k, v in s2s._weights.items()}
        self.V = s2s.voc_size
        self.step, self.soft_steps, self.options, self.released = 0, [], {}, 0

    def set_option(self, key, value):
        self.options[key] = value

    def train_begin(self, *adam, frozen=()):
        pass

    def set_train_state(self, m, v, step):
        self.step = step

    def train_step(self, idx, val, dec_in, dec_out, w, masks=None, mode=1):
        self.step += mode == 1
        return 1.0 / (1 + self.step), 0.0

    def train_step_soft(self, idx, val, dec_in, soft_idx, soft_q, w, masks=None, mode=1):
        assert mode == 1 and soft_idx.shape == soft_q.shape == dec_in.shape + (soft_idx.shape[2],)
        self.soft_steps.append(soft_idx.shape[2])
        self.step += 1
        return 1.0 / (1 + self.step), 0.0

    def score_targets(self, idx, val, dec_in, dec_out, want_align=False):
        self.shape = dec_out.shape

    def score_alternatives(self, K, want_entropy=True):
        assert want_entropy is False
        alt = np.broadcast_to(np.arange(1, K + 1, dtype=np.int32), self.shape + (K,)).copy()
        return alt, np.full(self.shape + (K,), np.log(1.0 / K), np.float32), None

    def score_release(self):
        self.released += 1

    def train_weights(self):
        return {k: np.array(v) for k, v in self.w.items()}

    def train_state(self):
        return {k: np.zeros_like(v) for k, v in self.w.items()}, {k: np.ones_like(v) for k, v in self.w.items()}, self.step

    def get_weights(self):
        return self.train_weights()

    def train_end(self):
        pass


def _corpus(tmp_path, alphabet='abcdef '):
    rng = np.random.default_rng(0)
    lines = [''.join(rng.choice(list(alphabet), size=rng.integers(3, 8))) for _ in range(200)]
    corpus = tmp_path / 'train.tsv'
    corpus.write_text(''.join('%s\t%s\n' % (l, l) for l in lines))
    return str(corpus)


def _model(monkeypatch, corpus, epochs=1, state=True, width=16, loaded=False):
    s2s = Sequence2Sequence(progbars=False)
    s2s.depth, s2s.width, s2s.batch_size, s2s.epochs, s2s.seed, s2s.checkpoint_training_state = 1, width, 16, epochs, 3, state
    s2s.configure()
    if loaded:                          # a teacher: the corpus' mapping, status 2
        s2s.map_files([corpus])
        s2s.status = 2
    eng = {}
    monkeypatch.setattr(s2s, '_require_engine', lambda: eng.setdefault('e', _StubEngine(s2s)))
    s2s._stub = eng
    return s2s


def test_teacher_with_another_mapping_is_refused_before_anything_runs(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    corpus = _corpus(tmp_path)
    (tmp_path / 'other').mkdir()
    other = _corpus(tmp_path / 'other', alphabet='abcdxy ')            # the same size, other characters
    teacher = _model(monkeypatch, other, loaded=True)
    student = _model(monkeypatch, corpus)
    with pytest.raises(ValueError, match='character mapping'):
        student.train([corpus], teacher=teacher)
    assert not student._stub and not teacher._stub                     # no engine was asked for
    (tmp_path / 'big').mkdir()
    bigger = _model(monkeypatch, _corpus(tmp_path / 'big', alphabet='abcdefgh '), loaded=True)
    with pytest.raises(ValueError, match='voc_size'):
        _model(monkeypatch, corpus).train([corpus], teacher=bigger)
    unloaded = _model(monkeypatch, corpus)
    with pytest.raises(ValueError, match='loaded'):
        _model(monkeypatch, corpus).train([corpus], teacher=unloaded)
    good = _model(monkeypatch, corpus, loaded=True)
    with pytest.raises(ValueError, match='distill_k'):
        _model(monkeypatch, corpus).train([corpus], teacher=good, distill_k=64)
    with pytest.raises(ValueError, match='distill_alpha'):
        _model(monkeypatch, corpus).train([corpus], teacher=good, distill_alpha=-0.1)
    assert not glob.glob('model.ckpt.*')


def test_distilled_checkpoints_record_k_and_alpha_and_resume_refuses_a_mismatch(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    corpus = _corpus(tmp_path)
    teacher = _model(monkeypatch, corpus, loaded=True)
    student = _model(monkeypatch, corpus)
    student.train([corpus], teacher=teacher, distill_k=3, distill_alpha=0.25)
    eng, teng = student._stub['e'], teacher._stub['e']
    assert eng.soft_steps and set(eng.soft_steps) == {4} and teng.released == 1 and teng.options['deterministic'] == 0
    (ck,) = glob.glob('model.ckpt.weights-01-*.h5')
    assert keras_h5.read_training_state(ck)['distill'] == (3, 0.25)
    with pytest.raises(ValueError, match='teacher is missing'):
        _model(monkeypatch, corpus, epochs=2).train([corpus], resume=ck)
    with pytest.raises(ValueError, match='distillation differs'):
        _model(monkeypatch, corpus, epochs=2).train([corpus], resume=ck, teacher=teacher, distill_k=4, distill_alpha=0.25)
    with pytest.raises(ValueError, match='distillation differs'):
        _model(monkeypatch, corpus, epochs=2).train([corpus], resume=ck, teacher=teacher, distill_k=3, distill_alpha=0.5)
    resumed = _model(monkeypatch, corpus, epochs=2)
    resumed.train([corpus], resume=ck, teacher=teacher, distill_k=3, distill_alpha=0.25)
    assert len(resumed.history) == 2 and resumed._stub['e'].soft_steps
    # a run without a teacher writes the keys it wrote before, and a teacher cannot join it later
    os.remove(ck)
    for f in glob.glob('model.ckpt.*'):
        os.remove(f)
    plain = _model(monkeypatch, corpus)
    plain.train([corpus])
    assert not plain._stub['e'].soft_steps
    (ck,) = glob.glob('model.ckpt.weights-01-*.h5')
    assert 'distill' not in keras_h5.read_training_state(ck)
    from cor_asv_ann_amd import hdf5
    with hdf5.File(ck) as f:
        assert 'distill_k' not in f['training_state'] and 'distill_alpha' not in f['training_state']
    with pytest.raises(ValueError, match='without a teacher'):
        _model(monkeypatch, corpus, epochs=2).train([corpus], resume=ck, teacher=teacher)


def test_the_abi_table_knows_the_new_entries():
    import cor_asv_ann_amd._native as nv
    assert len(nv.SIGNATURES['casv_train_step_soft'][1]) == 18 and len(nv.SIGNATURES['casv_debug_soft_ce_rows'][1]) == 14
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'cor_asv_ann_hip.h')) as f:
        header = f.read()
    assert 'int casv_train_step_soft(' in header and 'int casv_debug_soft_ce_rows(' in header
