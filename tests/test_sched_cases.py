"""Scheduled sampling on the CPU (tests/sched_cases.py): the coins against the generator's known answers, the definition on the
constructed rows, the float32 oracle against the float64 oracle within the left-out cap for every step case, the passes / prefix
property and the sequential equivalence on the oracle, and train(sample_schedule=...) with a stub engine."""
import glob
import math
import os

import numpy as np
import pytest

from cor_asv_ann_amd import keras_h5, training
from cor_asv_ann_amd.seq2seq import Sequence2Sequence
from tests import sample_cases as sa
from tests import sched_cases as sc


# ---- the generator and the definition ----
def test_coins_are_words_0_and_1_of_the_generator():
    for counter, key, words in sa.KNOWN_ANSWERS:
        seed, step_id = key[0] | (key[1] << 32), counter[0] | (counter[1] << 32)
        c, u2 = sc.coins(seed, step_id, counter[2], counter[3])
        assert float(c) == (words[0] >> 8) * 2.0 ** -24 and float(u2) == (words[1] >> 8) * 2.0 ** -24
    # every part of (seed, step_id, b, u) enters, the upper half of step_id too
    base = sc.coins(7, 5, 3, 2)
    for other in ((8, 5, 3, 2), (7, 5 + (1 << 32), 3, 2), (7, 6, 3, 2), (7, 5, 4, 2), (7, 5, 3, 3), (7 + (1 << 40), 5, 3, 2)):
        assert sc.coins(*other) != base
    c, _ = sc.coins(11, 1 << 33, np.arange(4000) % 50, np.arange(4000) // 50)
    assert 0.45 < (c < 0.5).mean() < 0.55 and c.min() >= 0 and c.max() < 1


@pytest.mark.parametrize('V', sc.KERNEL_V)
def test_definition_on_the_constructed_rows(V):
    rows = sc.constructed_rows(V)
    x = np.stack([r[1] for r in rows])
    gold, u = np.array([r[2] for r in rows]), np.array([r[3] for r in rows])
    b = np.arange(len(rows))
    for pick in ('greedy', 'sample'):
        one = sc.mix_rows(x, gold, b, u, 3, 4, 1.0, pick)
        zero = sc.mix_rows(x, gold, b, u, 3, 4, 0.0, pick)
        assert np.array_equal(zero['mix'], gold) and one['coin'].all() and not zero['coin'].any()
        for (name, _, g, _, fact), mix in zip(rows, one['mix']):
            if fact == 'gold':
                assert mix == g, (pick, name)
            elif pick == 'greedy':
                assert mix == fact, (pick, name)
            else:
                assert 1 <= mix < V and np.isfinite(x[[n for n, *_ in rows].index(name), mix]), (pick, name)


@pytest.mark.parametrize('V', sc.KERNEL_V)
def test_random_rows_leave_few_draws_out(V):
    """The kernel-alone rows: left_out's rule (float32 weights against float64 ones on the same float32 logits) takes at most
    LEFT_OUT_CAP of the replaced rows' draws, and the coins replace some rows and spare others."""
    x, gold, b, u = sc.random_rows(V)
    mark = np.where(gold >= 0, 0, -1)
    left = n = 0
    for seed, step_id in sc.KERNEL_GRID:
        for pick, tau in sc.KERNEL_DRAWS[1:]:
            want = sc.mix_rows(x, mark, b, u, seed, step_id, 0.5, pick, tau)
            assert 0 < want['replaced'].sum() < (want['eligible']).sum()
            out = sc.sampled_left_out(x.astype(np.float64), x, want['u2'], tau)
            left += int((out & want['replaced']).sum()); n += int(want['replaced'].sum())
    assert left <= sc.LEFT_OUT_CAP * n, (left, n)


# ---- the step's cases on the oracle ----
@pytest.mark.parametrize('case', sc.STEP_CASES, ids=sc.STEP_IDS)
def test_float32_oracle_follows_the_float64_oracle_within_the_cap(case):
    """Two passes at ratio 0.5, greedy and sampled: along the float64 oracle's mixes, the float32 oracle's pick differs from the
    float64 one only at positions the rule leaves out, and those stay within LEFT_OUT_CAP of the case's positions."""
    gold = sc.build(case)[3][2]
    for pick, tau in (('greedy', 1.0), ('sample', 1.0), ('sample', 0.5)):
        cur = gold
        replaced = 0
        for p in range(2):
            m64, out = sc.next_mix(case, cur, gold, 0.5, pick, tau)
            m32, _ = sc.next_mix(case, cur, gold, 0.5, pick, tau, dtype=np.float32)
            print('%s %s tau %g pass %d: %d of %d positions left out, %d replaced' % (case[0], pick, tau, p + 1, out.sum(), out.size, (m64 != gold).sum()))
            assert np.array_equal(m32[~out], m64[~out])
            assert out.sum() <= sc.LEFT_OUT_CAP * out.size, (pick, tau, p, int(out.sum()), out.size)
            assert np.array_equal(m64[:, 0], gold[:, 0]) and np.array_equal(m64[gold < 0], gold[gold < 0])
            replaced += int((m64 != gold).sum())
            cur = m64
        assert replaced > 0                 # (the case exercises the pick at all)


def test_passes_reach_the_sequential_procedure_position_by_position():
    """With P passes the positions u <= P of the parallel procedure's input are the sequential procedure's; with P >= U - 1 the two
    coincide.  The case has no position near a tie, so the device can be held to it exactly."""
    case = sc.SEQ_CASE
    gold = sc.build(case)[3][2]
    U = gold.shape[1]
    assert U == 6
    seq, out = sc.sequential(case, gold, 0.5)
    assert not out.any()
    assert (seq != gold).sum() >= 3
    mixes, outs = sc.parallel(case, gold, 0.5, U - 1)
    assert not any(o.any() for o in outs)
    for p, mix in enumerate(mixes, start=1):
        assert np.array_equal(mix[:, :p + 1], seq[:, :p + 1]), p
    assert np.array_equal(mixes[-1], seq)
    assert any(not np.array_equal(mixes[0], m) for m in mixes[1:])            # (the passes are not all the first: the property says something)
    again, _ = sc.next_mix(case, seq, gold, 0.5)
    assert np.array_equal(again, seq)       # a fixed point


# ---- the schedules ----
def test_schedule_ratios_at_known_epochs():
    r = training.schedule_ratio
    assert [r('linear', e, 10) for e in (0, 1, 2, 4, 5, 9)] == [0.0, 0.0, 3 / 9, 1.0, 1.0, 1.0]
    assert r('linear', 1, 1) == 0.0 and r('linear', 0, 1) == 0.0
    assert r('sigmoid', 0, 10) == 0.0 and r('exponential', 0, 10) == 0.0
    assert r('sigmoid', 1, 10) == 1 / (1 + math.exp(5 - 3.0)) and abs(r('sigmoid', 5, 30) - 0.5) < 1e-12
    assert r('exponential', 1, 10) == 1 - 0.9 ** 15.0 and r('exponential', 2, 300) == 1 - 0.9 ** 1.0
    assert r(0.25, 0, 10) == r(0.25, 7, 10) == 0.25
    assert r(lambda e: e / 4, 3, 10) == 0.75
    for bad in (lambda e: 1.5, lambda e: -0.1, lambda e: float('nan')):
        with pytest.raises(ValueError, match='ratio'):
            r(bad, 1, 10)
    assert training.schedule_name('sigmoid') == 'sigmoid' and training.schedule_name(0.25) == 'const:0.25'
    assert training.schedule_name(lambda e: 0.0) == 'callable'


# ---- train(sample_schedule=...): the checks, with a stub engine ----
class _StubEngine(object):
    """What train() asks of HipEngine on the host; a sampled step counts as a step and records what it was called with."""

    def __init__(self, s2s):
        self.w = {k: np.array(v) for k, v in s2s._weights.items()}
        self.pshapes = {k: v.shape for k, v in self.w.items()}
        self.step, self.sampled, self.hard, self.options = 0, [], 0, {}

    def set_option(self, key, value):
        self.options[key] = value

    def train_begin(self, *adam, frozen=()):
        pass

    def set_train_state(self, m, v, step):
        self.step = step

    def train_step(self, idx, val, dec_in, dec_out, w, masks=None, mode=1):
        self.step += mode == 1
        self.hard += mode == 1
        return 1.0 / (1 + self.step), 0.0

    def train_step_sampled(self, idx, val, dec_in, dec_out, w, masks=None, mode=1, **kw):
        assert mode == 1 and kw['step_id'] == self.step       # the session's step count
        self.sampled.append(kw)
        self.step += 1
        return 1.0 / (1 + self.step), 0.0, np.repeat(dec_in[None], kw['passes'], axis=0)

    def train_weights(self):
        return {k: np.array(v) for k, v in self.w.items()}

    def train_state(self):
        return {k: np.zeros_like(v) for k, v in self.w.items()}, {k: np.ones_like(v) for k, v in self.w.items()}, self.step

    def get_weights(self):
        return self.train_weights()

    def train_end(self):
        pass


def _corpus(tmp_path):
    rng = np.random.default_rng(0)
    lines = [''.join(rng.choice(list('abcdef '), size=rng.integers(3, 8))) for _ in range(200)]
    corpus = tmp_path / 'train.tsv'
    corpus.write_text(''.join('%s\t%s\n' % (l, l) for l in lines))
    return str(corpus)


def _model(monkeypatch, epochs=1):
    s2s = Sequence2Sequence(progbars=False)
    s2s.depth, s2s.width, s2s.batch_size, s2s.epochs, s2s.seed, s2s.checkpoint_training_state = 1, 16, 16, epochs, 3, True
    s2s.configure()
    eng = {}
    monkeypatch.setattr(s2s, '_require_engine', lambda: eng.setdefault('e', _StubEngine(s2s)))
    s2s._stub = eng
    return s2s


def test_sampling_keywords_are_checked_before_anything_runs(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    corpus = _corpus(tmp_path)
    for kw, match in ((dict(sample_schedule='cosine'), 'sample_schedule'), (dict(sample_schedule=1.5), 'ratio in'),
                      (dict(sample_schedule=float('nan')), 'ratio in'), (dict(sample_schedule=[0.5]), 'sample_schedule'),
                      (dict(sample_schedule='linear', sample_pick='beam'), 'sample_pick'),
                      (dict(sample_schedule='linear', sample_passes=0), 'sample_passes'),
                      (dict(sample_schedule='linear', sample_passes=9), 'sample_passes'),
                      (dict(sample_schedule='linear', sample_passes=1.5), 'sample_passes'),
                      (dict(sample_schedule='linear', sample_pick='sample', sample_temperature=0.0), 'sample_temperature'),
                      (dict(sample_schedule='linear', sample_temperature=float('inf')), 'sample_temperature'),
                      (dict(sample_schedule='linear', teacher=object()), 'teacher')):
        s2s = _model(monkeypatch)
        with pytest.raises(ValueError, match=match):
            s2s.train([corpus], **kw)
        assert not s2s._stub, kw                # no engine was asked for
    assert not glob.glob('model.ckpt.*')
    # the attribute of the reference stays refused, and says where to go
    s2s = Sequence2Sequence(progbars=False)
    s2s.scheduled_sampling = 'linear'
    with pytest.raises(NotImplementedError, match='sample_schedule'):
        s2s.configure()


def test_sampled_run_records_its_settings_and_resume_refuses_a_mismatch(tmp_path, monkeypatch, caplog):
    monkeypatch.chdir(tmp_path)
    corpus = _corpus(tmp_path)
    first = _model(monkeypatch, epochs=3)
    first.epochs = 3
    import logging
    with caplog.at_level(logging.INFO):
        # (three epochs of 'exponential': 0, then 1 - 0.9 ** 50, 1 - 0.9 ** 100)
        first.train([corpus], sample_schedule='exponential', sample_pick='sample', sample_passes=2, sample_temperature=0.5)
    assert 'sample ratio 0.0000' in caplog.text and 'sample ratio %.4f' % (1 - 0.9 ** 50) in caplog.text
    eng = first._stub['e']
    per_epoch = len(eng.sampled) // 3
    assert eng.hard == 0 and per_epoch >= 2 and len(eng.sampled) == 3 * per_epoch
    assert [k['step_id'] for k in eng.sampled] == list(range(len(eng.sampled)))
    assert {k['ratio'] for k in eng.sampled[:per_epoch]} == {0.0}
    assert {k['ratio'] for k in eng.sampled[per_epoch:2 * per_epoch]} == {1 - 0.9 ** 50}
    seeds = {k['seed'] for k in eng.sampled}
    assert len(seeds) == 1 and all(k['pick'] == 'sample' and k['passes'] == 2 and k['temperature'] == 0.5 for k in eng.sampled)
    (seed,) = seeds
    (ck,) = glob.glob('model.ckpt.weights-01-*.h5')
    assert keras_h5.read_training_state(ck)['sample'] == dict(seed=seed, schedule='exponential', pick='sample', passes=2, temperature=0.5)
    good = dict(sample_schedule='exponential', sample_pick='sample', sample_passes=2, sample_temperature=0.5)
    for change, match in ((dict(sample_schedule='linear'), 'schedule differs'), (dict(sample_pick='greedy'), 'pick differs'),
                          (dict(sample_passes=1), 'passes differs'), (dict(sample_temperature=1.0), 'temperature differs'),
                          (dict(sample_schedule=None), 'trained with the sample schedule')):
        with pytest.raises(ValueError, match=match):
            _model(monkeypatch, epochs=3).train([corpus], resume=ck, **dict(good, **change))
    # a resumed run keeps the seed and goes on counting steps where the checkpoint's session stood
    resumed = _model(monkeypatch, epochs=3)
    resumed.train([corpus], resume=ck, **good)
    again = resumed._stub['e'].sampled
    assert len(again) == 2 * per_epoch and [k['step_id'] for k in again] == list(range(per_epoch, 3 * per_epoch))
    assert {k['seed'] for k in again} == {seed} and again[0]['ratio'] == 1 - 0.9 ** 50
    # a plain run writes the keys it wrote before, and a schedule cannot join it later
    for f in glob.glob('model.ckpt.*'):
        os.remove(f)
    plain = _model(monkeypatch)
    plain.train([corpus])
    assert plain._stub['e'].hard and not plain._stub['e'].sampled
    (ck,) = glob.glob('model.ckpt.weights-01-*.h5')
    assert 'sample' not in keras_h5.read_training_state(ck)
    with pytest.raises(ValueError, match='without a sample schedule'):
        _model(monkeypatch, epochs=2).train([corpus], resume=ck, sample_schedule=0.5)


def test_the_abi_table_knows_the_new_entries():
    import ctypes
    import cor_asv_ann_amd._native as nv
    assert len(nv.SIGNATURES['casv_train_step_sampled'][1]) == 18 and len(nv.SIGNATURES['casv_debug_sched_rows'][1]) == 10
    assert ctypes.sizeof(nv.SchedParams) == 32
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'cor_asv_ann_hip.h')) as f:
        header = f.read()
    assert 'int casv_train_step_sampled(' in header and 'int casv_debug_sched_rows(' in header and '} casv_sched_params;' in header
