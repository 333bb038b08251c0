"""The minimum-risk head's definition and its host side without a device: tests/risk_cases.py's numpy head against a finite
difference of its own loss, its invariants, the wrong heads against the bounds, the whole-step reference that
tests/test_gpu_risk.py compares the device with, train()'s checks and risk_step's slicing against stubs."""
import glob
import os

import numpy as np
import pytest

from cor_asv_ann_amd import keras_h5, training
from cor_asv_ann_amd.seq2seq import Sequence2Sequence
from tests import risk_cases as rc

FD_CASES = [c for c in rc.HEAD_CASES if c[0] == 5 and c[1] in (2, 3)]


# ---- the definition ----
@pytest.mark.parametrize('case', FD_CASES, ids=lambda c: 'V%d_N%d_G%d_U%d' % c)
def test_dlogits_are_the_gradient_of_the_loss(case):
    """head(float64)'s dlogits = a central finite difference of its own loss in every logit: relative 1e-6 at a step of 1e-5
    (float64, a smooth function)."""
    (x, target, weight, cost, alpha, _), f64, _ = rc.reference(case)
    V, N, G, U = case
    d = f64[1]
    x64 = np.asarray(x, np.float64)
    h = 1e-5
    fd = np.zeros_like(d)
    for i in np.ndindex(x64.shape):
        up, down = x64.copy(), x64.copy()
        up[i] += h
        down[i] -= h
        fd[i] = (rc.head(up, target, weight, cost, alpha, N)[0] - rc.head(down, target, weight, cost, alpha, N)[0]) / (2 * h)
    assert np.abs(fd - d).max() <= 1e-6 * max(np.abs(d).max(), 1e-300), (np.abs(fd - d).max(), np.abs(d).max())


@pytest.mark.parametrize('case', rc.HEAD_CASES, ids=lambda c: 'V%d_N%d_G%d_U%d' % c)
def test_invariants_of_the_head(case):
    """The c of a group sum to zero within N * 2^-52 * alpha * max cost; the q of a group with a member sum to 1; N = 1 gives
    exactly zero coefficients and loss = mean cost; rows of zero kind have zero gradient rows."""
    (x, target, weight, cost, alpha, kinds), (loss, d, q, c), _ = rc.reference(case)
    V, N, G, U = case
    inv = 1.0 / max(sum(1 for g in range(G) if (cost[g * N:(g + 1) * N] >= 0).any()), 1)
    for g in range(G):
        rows = slice(g * N, (g + 1) * N)
        members = cost[rows] >= 0
        assert abs(c[rows].sum()) <= N * 2.0 ** -52 * alpha * max(float(cost[rows].max()), 0.0) * inv, (g, c[rows].sum())
        assert not q[rows][~members].any() and not c[rows][~members].any()
        if members.any():
            assert abs(q[rows].sum() - 1.0) <= N * 2.0 ** -52
    assert not d[(target < 0) | (weight == 0) | (cost < 0)[:, None]].any()
    if N == 1:
        assert not c.any() and not d.any()
        members = cost[cost >= 0].astype(np.float64)
        assert loss == pytest.approx(members.mean() if len(members) else 0.0, rel=1e-15, abs=0.0)


@pytest.mark.parametrize('wrong', rc.WRONG_HEADS)
def test_every_wrong_head_misses_a_bound_fourfold(wrong):
    """Each mistake misses head(float64) on at least one case by 4 x the coefficient bound (q or coef, given the same logp) or
    4 x the noise bound (loss or dlogits)."""
    worst = 0.0
    for case in rc.HEAD_CASES:
        (x, target, weight, cost, alpha, _), f64, f32 = rc.reference(case)
        V, N, G, U = case
        pad = ((V + 31) & ~31) - V
        bad = rc.head(x, target, weight, cost, alpha, N, np.float64, wrong=wrong, pad=pad)
        cb = rc.coef_bound(cost, alpha, N)
        bound = rc.bounds(f32, f64, coef_floor=cb)
        err = rc.errors(bad, f64)
        worst = max(worst, err[0] / bound[0], err[1] / bound[1])
        if cb:
            worst = max(worst, float(np.abs(bad[2] - f64[2]).max()) / cb, float(np.abs(bad[3] - f64[3]).max()) / cb)
    assert worst >= 4.0, (wrong, worst)


def test_the_constants_come_from_the_measurement():
    assert rc.C >= 2 * rc.MEASURED_MAX_RATIO and rc.C == float(np.ceil(2 * rc.MEASURED_MAX_RATIO))
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'risk_head_noise.txt')
    with open(path) as f:
        assert 'largest noise ratio %.3f' % rc.MEASURED_MAX_RATIO in f.read()


@pytest.mark.parametrize('name', sorted(rc.STEP_CASES))
def test_the_whole_step_reference(name):
    """The reference the device's step is held to, in float32 and float64: the members' target probabilities lie inside (1e-6,
    1 - 1e-6) -- where the oracle's clipped cross-entropy backward is this head's --, the two precisions agree, a line that is
    not a member gets no weight, and the gradient is the risk's: a central difference of the float64 risk along a random
    direction of the weights equals the gradient's product with it -- the gradient less the regulariser's, which the oracle adds
    by a rule of its own (its gradients with all weights zero) and the device shares."""
    from oracle.train import forward_backward
    case, cfg, w, inputs, batch, N, cost = rc.step_inputs(name)
    B = case[4]
    assert B % N == 0 and B // N == 2 and len(cost) == B
    o64, p64 = rc.step_reference(cfg, w, inputs, N, cost, rc.STEP_ALPHA, np.float64)
    o32, p32 = rc.step_reference(cfg, w, inputs, N, cost, rc.STEP_ALPHA, np.float32)
    for lo, hi in (p64, p32):
        assert 1e-6 < lo and hi < 1 - 1e-6, (lo, hi)
    assert abs(o32[0] - o64[0]) <= 1e-5 * abs(o64[0]) and abs(o32[1] - o64[1]) <= 1e-4 * o64[1]
    if name == 'd3_w64_b8_m':
        assert (cost < 0).sum() == 1

    def risk(weights):
        enc_in, dec_in, dec_out, wts, masks = inputs
        cast = lambda a: np.asarray(a, np.float64)
        m = {'enc': [cast(a) for a in masks['enc']], 'dec': [cast(a) for a in masks['dec']], 'cell': cast(masks['cell'])}
        _, _, aux = forward_backward(cfg, weights, cast(enc_in), cast(dec_in), cast(dec_out), cast(wts), m, want_grads=False,
                                     window_dtype=np.float32)
        y = np.asarray(dec_out)
        target = np.where(y.any(axis=2), y.argmax(axis=2), -1)
        pt = np.take_along_axis(aux['probs'], np.where(target >= 0, target, 0)[:, :, None], axis=2)[:, :, 0]
        logp = np.where(target >= 0, np.log(np.where(target >= 0, pt, 1)), 0)
        return rc.coefficients(logp, target, wts, cost, rc.STEP_ALPHA, N)[0]
    rng = np.random.default_rng(5)
    w64 = {k: np.asarray(v, np.float64) for k, v in w.items()}
    direction = {k: rng.normal(size=v.shape) for k, v in w64.items()}
    h = 1e-6
    up = risk({k: v + h * direction[k] for k, v in w64.items()})
    down = risk({k: v - h * direction[k] for k, v in w64.items()})
    enc_in, dec_in, dec_out, wts, masks = inputs
    cast = lambda a: np.asarray(a, np.float64)
    m64 = {'enc': [cast(a) for a in masks['enc']], 'dec': [cast(a) for a in masks['dec']], 'cell': cast(masks['cell'])}
    _, reg_only, _ = forward_backward(cfg, w64, cast(enc_in), cast(dec_in), cast(dec_out), cast(wts) * 0, m64, window_dtype=np.float32)
    slope = sum(float(((o64[2][k] - reg_only[k]) * direction[k]).sum()) for k in w64)
    assert abs((up - down) / (2 * h) - slope) <= 1e-6 * abs(slope), ((up - down) / (2 * h), slope)


# ---- the host side ----
class _Stub(object):
    """A model's stand-in for check_risk and risk_step."""
    def __init__(self, batch_size=8, voc=None, status=2):
        self.batch_size, self.status = batch_size, status
        chars = voc or 'abc\n'
        self.mapping = ({c: i + 1 for i, c in enumerate(chars)}, {i + 1: c for i, c in enumerate(chars)})
        self.voc_size = len(chars) + 1


def test_check_risk_refuses_what_the_keywords_rule_out():
    s2s = _Stub()
    ok = dict(risk_samples=4, risk_alpha=1.0, risk_temperature=1.0, risk_top_k=0, risk_top_p=1.0, proposal=None, teacher=None,
              sample_schedule=None)
    training.check_risk(s2s, **ok)
    training.check_risk(s2s, **dict(ok, proposal=_Stub()))
    bad = [(dict(teacher=object()), 'teacher'), (dict(sample_schedule='linear'), 'sample_schedule'), (dict(risk_samples=1), 'risk_samples'),
           (dict(risk_samples=65), 'risk_samples'), (dict(risk_samples=2.5), 'risk_samples'), (dict(risk_samples=9), 'batch_size'),
           (dict(risk_alpha=0.0), 'risk_alpha'), (dict(risk_alpha=float('nan')), 'risk_alpha'), (dict(risk_alpha=float('inf')), 'risk_alpha'),
           (dict(risk_temperature=-1.0), 'risk_temperature'), (dict(risk_top_k=-1), 'risk_top_k'), (dict(risk_top_p=0.0), 'risk_top_p'),
           (dict(proposal=s2s), 'another model'), (dict(proposal=_Stub(status=1)), 'loaded'),
           (dict(proposal=_Stub(voc='abcd\n')), 'voc_size'), (dict(proposal=_Stub(voc='abd\n')), 'character mapping')]
    for change, match in bad:
        with pytest.raises(ValueError, match=match):
            training.check_risk(s2s, **dict(ok, **change))


def test_check_risk_resume_refuses_other_settings():
    mine = {'samples': 4, 'alpha': 0.5, 'temperature': 1.0, 'top_k': 0, 'top_p': 1.0, 'own_proposal': True, 'seed': 7}
    training.check_risk_resume({'risk': dict(mine)}, 'f', dict(mine, seed=8))          # (the seed is the file's)
    training.check_risk_resume({}, 'f', None)
    with pytest.raises(ValueError, match='without risk_samples'):
        training.check_risk_resume({}, 'f', mine)
    with pytest.raises(ValueError, match='risk_samples=4'):
        training.check_risk_resume({'risk': mine}, 'f', None)
    for key, value in (('samples', 8), ('alpha', 1.0), ('temperature', 0.5), ('top_k', 5), ('top_p', 0.9), ('own_proposal', False)):
        with pytest.raises(ValueError, match='risk %s differs' % key):
            training.check_risk_resume({'risk': mine}, 'f', dict(mine, **{key: value}))


class _Proposal(object):
    """Draws fixed lines: per source 'ab\\n' (a duplicate of the gold line of source 0), the gold line again, 'b\\n'."""
    def __init__(self):
        self.calls = []

    def sample_lines(self, lines, conf=None, n=1, temperature=1.0, top_k=0, seed=None, streams=None, alignments=False, top_p=1.0):
        self.calls.append((list(lines), n, temperature, top_k, seed, list(streams), top_p))
        return [[['ab\n', 'ab\n', 'b\n'][:n] for _ in lines]] + [None] * 4

    def consensus_of(self, candidates, weights=None, normalise=False, distances=False):
        def lev(a, b):
            row = list(range(len(b) + 1))
            for i, ca in enumerate(a, 1):
                row, prev = [i] + [0] * len(b), row
                for j, cb in enumerate(b, 1):
                    row[j] = min(prev[j] + 1, row[j - 1] + 1, prev[j - 1] + (ca != cb))
            return row[-1]
        assert distances and not normalise and weights is None
        return None, None, [[[lev(a, b) for b in cands] for a in cands] for cands in candidates]


class _Engine(object):
    def __init__(self):
        self.steps = []

    def train_step_risk(self, idx, val, dec_in, dec_out, w, cost, n, alpha, masks=None, mode=1):
        self.steps.append((idx.copy(), dec_in.copy(), dec_out.copy(), w.copy(), np.array(cost), n, alpha, masks, mode))
        return 0.25 * len(self.steps), 0.0


def test_risk_step_slices_the_batch_and_removes_duplicates():
    s2s = Sequence2Sequence(progbars=False)
    s2s.mapping = ({'': 0, '\n': 1, 'a': 2, 'b': 3, 'c': 4}, {0: '', 1: '\n', 2: 'a', 3: 'b', 4: 'c'})
    s2s.voc_size, s2s.dropout, s2s.width, s2s.depth = 5, 0.0, 16, 1
    src = ['ab\n', 'abc\n', 'c\n', 'ba\n', 'bb\n']
    tgt = ['ab\n', 'abcc\n', 'b\n', 'ba\n', 'bb\n']
    settings = {'samples': 4, 'alpha': 0.5, 'temperature': 0.7, 'top_k': 3, 'top_p': 0.9, 'seed': 99, 'own_proposal': True,
                'model': s2s, 'batch_size': 8, 'stream': 1000}
    proposal, engine = _Proposal(), _Engine()
    losses = training.risk_step(engine, proposal, (src, None, tgt), settings, np.random.default_rng(1))
    # 8 // 4 = 2 sources per slice: slices of 2, 2 and 1 sources, never more than 8 decoder rows
    assert losses == [0.25, 0.5, 0.75] and [len(s[0]) for s in engine.steps] == [8, 8, 4]
    assert [c[0] for c in proposal.calls] == [src[0:2], src[2:4], src[4:5]]
    assert [c[5] for c in proposal.calls] == [[1000, 1001], [1002, 1003], [1004]] and settings['stream'] == 1005
    assert all(c[1:5] == (3, 0.7, 3, 99) and c[6] == 0.9 for c in proposal.calls)
    idx, dec_in, dec_out, w, cost, n, alpha, masks, mode = engine.steps[0]
    assert (n, alpha, masks, mode) == (4, 0.5, None, 1)
    # source 0: gold 'ab\n', then 'ab\n' twice (duplicates of the gold line: not members), then 'b\n' at distance 1 of 3
    assert cost[:4].tolist() == [0.0, -1.0, -1.0, pytest.approx(1 / 3)]
    # source 1: gold 'abcc\n' (5 long), 'ab\n' at distance 2, its duplicate, 'b\n' at distance 3
    assert cost[4:].tolist() == [0.0, pytest.approx(2 / 5), -1.0, pytest.approx(3 / 5)]
    # the rows of a group share the source; the candidates are the targets, gold first
    assert all(np.array_equal(idx[g * 4 + i], idx[g * 4]) for g in range(2) for i in range(4))
    assert dec_out[0, :3].tolist() == [2, 3, 1] and dec_out[3, :3].tolist() == [3, 1, -1] and dec_out[4, :5].tolist() == [2, 3, 4, 4, 1]
    assert dec_in[4, :5].tolist() == [-1, 2, 3, 4, 4] and np.array_equal(w, (dec_out >= 0).astype(np.float32))


# ---- train() ----
class _StubEngine(object):
    def __init__(self, s2s):
        self.pshapes = {k: v.shape for k, v in s2s._weights.items()}
        self.w = {k: np.array(v) for k, v in s2s._weights.items()}
        self.step, self.risk_steps, self.options = 0, [], {}

    def set_option(self, key, value):
        self.options[key] = value

    def train_begin(self, *adam, frozen=()):
        pass

    def set_train_state(self, m, v, step):
        self.step = step

    def train_step(self, idx, val, dec_in, dec_out, w, masks=None, mode=1):
        self.step += mode == 1
        return 1.0 / (1 + self.step), 0.0

    def train_step_risk(self, idx, val, dec_in, dec_out, w, cost, n, alpha, masks=None, mode=1):
        assert mode == 1 and len(cost) == len(idx) and len(idx) % n == 0 and len(idx) <= 16
        self.risk_steps.append((len(idx), n, alpha))
        self.step += 1
        return 0.5, 0.0

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


def _model(monkeypatch, corpus, epochs=1, loaded=False):
    s2s = Sequence2Sequence(progbars=False)
    s2s.depth, s2s.width, s2s.batch_size, s2s.epochs, s2s.seed, s2s.checkpoint_training_state = 1, 16, 16, epochs, 3, True
    s2s.configure()
    if loaded:
        s2s.map_files([corpus])
        s2s.status = 2
        monkeypatch.setattr(s2s, 'sample_lines', lambda lines, conf=None, n=1, **kw: [[[line] * n for line in lines]] + [None] * 4)
        monkeypatch.setattr(s2s, 'consensus_of', lambda cands, distances=False: (None, None, [[[0] * len(c) for _ in c] for c in cands]))
    eng = {}
    monkeypatch.setattr(s2s, '_require_engine', lambda: eng.setdefault('e', _StubEngine(s2s)))
    s2s._stub = eng
    return s2s


def test_train_refuses_bad_risk_keywords_before_anything_runs(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    corpus = _corpus(tmp_path)
    proposal = _model(monkeypatch, corpus, loaded=True)
    for kw, match in ((dict(risk_samples=4, teacher=proposal), 'teacher'), (dict(risk_samples=4, sample_schedule='linear'), 'sample_schedule'),
                      (dict(risk_samples=17), 'batch_size'), (dict(risk_samples=1), 'risk_samples'), (dict(risk_samples=4, risk_alpha=0), 'risk_alpha'),
                      (dict(proposal=proposal), 'without risk_samples')):
        student = _model(monkeypatch, corpus)
        with pytest.raises(ValueError, match=match):
            student.train([corpus], **kw)
        assert not student._stub
    assert not glob.glob('model.ckpt.*')


def test_risk_checkpoints_record_the_settings_and_resume_refuses_a_mismatch(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    corpus = _corpus(tmp_path)
    proposal = _model(monkeypatch, corpus, loaded=True)
    student = _model(monkeypatch, corpus)
    student.train([corpus], risk_samples=4, risk_alpha=0.5, proposal=proposal)
    steps = student._stub['e'].risk_steps
    assert steps and all(rows <= 16 and n == 4 and alpha == 0.5 for rows, n, alpha in steps)
    (ck,) = glob.glob('model.ckpt.weights-01-*.h5')
    recorded = keras_h5.read_training_state(ck)['risk']
    assert {k: recorded[k] for k in ('samples', 'alpha', 'temperature', 'top_k', 'top_p', 'own_proposal')} == {
        'samples': 4, 'alpha': 0.5, 'temperature': 1.0, 'top_k': 0, 'top_p': 1.0, 'own_proposal': False} and 'seed' in recorded
    with pytest.raises(ValueError, match='risk alpha differs'):
        _model(monkeypatch, corpus, epochs=2).train([corpus], resume=ck, risk_samples=4, risk_alpha=1.0, proposal=proposal)
    with pytest.raises(ValueError, match='trained with risk_samples'):
        _model(monkeypatch, corpus, epochs=2).train([corpus], resume=ck)
    resumed = _model(monkeypatch, corpus, epochs=2)
    resumed.train([corpus], resume=ck, risk_samples=4, risk_alpha=0.5, proposal=proposal)
    assert len(resumed.history) == 2 and resumed._stub['e'].risk_steps
    for f in glob.glob('model.ckpt.*'):
        os.remove(f)
    plain = _model(monkeypatch, corpus)
    plain.train([corpus], risk_samples=0)
    assert not plain._stub['e'].risk_steps
    (ck,) = glob.glob('model.ckpt.weights-01-*.h5')
    assert 'risk' not in keras_h5.read_training_state(ck)
    from cor_asv_ann_amd import hdf5
    with hdf5.File(ck) as f:
        assert 'risk' not in f['training_state']
    with pytest.raises(ValueError, match='without risk_samples'):
        _model(monkeypatch, corpus, epochs=2).train([corpus], resume=ck, risk_samples=4, proposal=proposal)


def test_the_abi_table_knows_the_new_entries():
    import cor_asv_ann_amd._native as nv
    assert len(nv.SIGNATURES['casv_train_step_risk'][1]) == 21 and len(nv.SIGNATURES['casv_debug_risk_rows'][1]) == 16
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'cor_asv_ann_hip.h')) as f:
        header = f.read()
    assert 'int casv_train_step_risk(' in header and 'int casv_debug_risk_rows(' in header
