"""The cases and references of tests/sample_cut_cases.py, held on the CPU: the restatement against a plain loop and against
sample_cases.draw_rows, the constructed rows' facts, the ambiguity cap of every kernel and model case on the reference alone, and the
host side of the feature -- sample_lines' routing, train()'s keywords and checkpoints, the ABI table and the header."""
import glob
import os

import numpy as np
import pytest

from tests import sample_cases as sa
from tests import sample_cut_cases as cu
from tests.decode_noise_cases import OLD_RT

U_SWEEP = np.concatenate([np.array([0.0, 1 - 2.0 ** -24]), (np.arange(30) + 0.5) / 30]).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ 1. the definition
def _nucleus_by_loop(x, tau, cut):
    """(a) and (b) for one row, one addition at a time in Python floats (float64)."""
    V = len(x)
    key = lambda v: (-float(x[v]) if x[v] != 0 else 0.0, v)          # x descending, -0 == +0, the lower index first
    order = sorted(range(1, V), key=key)
    top_k, top_p = cut
    n_a = top_k if 0 < top_k < V - 1 else V - 1
    if not np.float32(top_p) < 1:
        return order[:n_a]
    mc = max(float(x[v]) for v in range(1, V))
    w = [float(np.exp((np.float64(x[v]) - mc) / np.float64(np.float32(tau)))) for v in order[:n_a]]
    chunk = (V + 63) // 64
    c = [0.0] * 64
    runs = []
    for l in range(64):
        run = 0.0
        for j in range(l * chunk, min(n_a, (l + 1) * chunk)):
            run += w[j]
            runs.append((l, run))
        c[l] = run
    off, acc = [], 0.0
    for l in range(64):
        off.append(acc)
        acc = acc + c[l]
    P = [off[l] + run for l, run in runs]
    target = float(np.float64(np.float32(top_p))) * P[n_a - 1]
    jstar = next(j for j in range(n_a) if P[j] >= target)
    return order[:jstar + 1]


@pytest.mark.parametrize('V', (2, 12, 40, 65, 130))
def test_restatement_equals_a_plain_loop(V):
    rng = np.random.default_rng(V)
    x = (rng.standard_normal((6, V)) * 2).astype(np.float32)
    x[1, V // 2:] = x[1, V // 2]                                 # ties
    x[2, 1::2] = -np.inf
    x[2, V - 1] = 0.5
    for cut in ((0, 0.5), (0, 0.9), (5, 0.9), (0, cu.SMALLEST_P), (V - 2, 0.7), (4095, 0.3), (3, 1.0)):
        for tau in (0.5, 1.0, 2.0):
            d = cu.draw_rows(x, np.full(6, 0.3, np.float32), tau, cut)
            for r in range(6):
                want = _nucleus_by_loop(x[r], tau, cut)
                assert d['n'][r] == len(want), (V, cut, tau, r)
                assert sorted(np.nonzero(d['cand'][r])[0].tolist()) == sorted(want), (V, cut, tau, r)


def test_consequences_of_the_definition():
    rng = np.random.default_rng(5)
    for V in (12, 40, 96):
        x = (rng.standard_normal((50, V)) * 2).astype(np.float32)
        u = rng.random(50).astype(np.float32)
        for tau in (0.5, 1.0):
            for k in (0, 1, 8, 64):                       # no nucleus: sample_cases' draw at top_k
                a, b = cu.draw_rows(x, u, tau, (k, 1.0)), sa.draw_rows(x, u, tau, k)
                assert all(np.array_equal(a[key], b[key], equal_nan=True) for key in b), (V, tau, k)
            a, b = cu.draw_rows(x, u, tau, (0, cu.SMALLEST_P)), sa.draw_rows(x, u, tau, 1)
            assert all(np.array_equal(a[key], b[key], equal_nan=True) for key in b) and (a['n'] == 1).all()
            d = cu.draw_rows(x, u, tau, (0, 0.8))         # the nucleus is never empty, never holds weight 0, and reaches its mass
            assert (d['n'] >= 1).all() and (d['cand'].sum(axis=1) == d['n']).all()
            kept = np.where(d['cand'], d['w'], 0).sum(axis=1)
            full = sa.draw_rows(x, u, tau, 0)['w'].sum(axis=1)
            assert (kept >= 0.8 * full * (1 - 1e-12)).all() and d['cand'][np.arange(50), d['idx']].all()


def test_constructed_rows_keep_their_facts():
    names = set()
    for name, x, cut, tau, facts in cu.constructed_rows():
        names.add(name)
        rows = np.repeat(x[None], len(U_SWEEP), axis=0)
        for dt in (np.float64, np.float32):
            d = cu.draw_rows(rows, U_SWEEP, tau, cut, dt)
            assert d['valid'].all() == facts['valid'] and d['valid'].any() == facts['valid'], (name, dt)
            if not facts['valid']:
                assert (d['idx'] == 1).all() and np.isnan(d['logq']).all()
                continue
            assert 0 not in d['idx'] and (x[d['idx']] > -np.inf).all(), name
            if 'only' in facts:
                assert set(d['idx'].tolist()) <= set(facts['only']), (name, dt, sorted(set(d['idx'].tolist())))
                assert set(np.nonzero(d['cand'][0])[0].tolist()) == set(facts['only']) or name in ('minus_inf_members_k8',), name
            if 'never' in facts:
                assert not set(d['idx'].tolist()) & set(facts['never']), name
    assert {'equal_p025', 'equal_k5_p05', 'maximum_alone', 'tie_at_the_border', 'mixed_zeros', 'minus_inf_members', 'index_0_largest', 'v2',
            'v640_k65', 'v640_k100', 'v640_k638', 'k_beyond_all', 'cold', 'plus_inf', 'all_minus_inf', 'nan_at_17'} <= names


# ------------------------------------------------------------------------------------------------------------------ 2. the caps
@pytest.mark.parametrize('c', cu.KERNEL_CASES, ids=cu.KERNEL_IDS)
def test_kernel_cases_stay_inside_the_cap_at_the_kernel_floor(c):
    """The measurement behind KERNEL_FLOOR: the float32 restatement against the float64 one, on the case's own rows and -- for
    statistics -- on 400 more of its kind: no different draw outside the margin, at most LEFT_OUT_CAP left out."""
    V, R, cut, tau, scale = c
    x, streams, samples, step, seed = cu.kernel_case(c)
    u = sa.uniform(seed, streams, samples, step)
    rng = np.random.default_rng(V + R)
    more = 400 if V <= 640 else 100
    x = np.concatenate([x, (rng.standard_normal((more, V)) * scale).astype(np.float32)])
    u = np.concatenate([u, rng.random(more).astype(np.float32)])
    d64, d32 = cu.draw_rows(x, u, tau, cut), cu.draw_rows(x, u, tau, cut, np.float32)
    lo, _ = cu.left_out(u, d64, d32, cu.KERNEL_FLOOR)
    print('%s: %d rows, %.2f %% left out at the floor 2^-20, %d nuclei differ' % (str(c), len(u), 100.0 * lo.mean(), int((d64['n'] != d32['n']).sum())))
    assert np.array_equal(d64['idx'][~lo], d32['idx'][~lo])
    assert lo[:R].sum() <= cu.cap_rows(R) and lo.mean() <= cu.LEFT_OUT_CAP


@pytest.mark.parametrize('case,tau,cut', cu.MODEL_DRAWS, ids=cu.MODEL_DRAW_IDS)
def test_reference_stays_inside_the_ambiguity_cap(case, tau, cut):
    ref = cu.reference_run(case, tau, cut, seed=2024)
    seq = ref['seq']
    reported = np.arange(seq.shape[1])[None, :] < sa.lengths(seq)[:, None]
    n, out, wrong, disagree, need = cu.compare_draws(ref, seq, tau, cut, reported)
    print('%s tau=%g cut=%r: %d draws, %.1f %% left out, %d o32/o64 disagreements outside the margin' % (case[0], tau, cut, n, 100.0 * out / n, disagree))
    assert n > 100 and out <= cu.LEFT_OUT_CAP * n
    assert wrong == 0 and disagree == 0 and need == 0.0


# ------------------------------------------------------------------------------------------------------------------ 3. the facade
def _stub_facade(batch_size):
    from tests.test_sample_cases import _StubEngine, _stub_facade as plain

    class Stub(_StubEngine):
        def decode_sample_cut(self, samples, temperature=1.0, top_k=0, top_p=1.0, seed=0, streams=None, steps=None, want_align=False):
            out = self.decode_sample(samples, temperature, top_k, seed, streams, steps, want_align)
            self.calls[-1].update(cut_entry=True, top_p=top_p)
            return out
    s2s = plain(batch_size)
    s2s.engine = Stub()
    return s2s


def test_sample_lines_routes_by_the_cut():
    from tests.test_sample_cases import LINES
    for kw, cut_entry in ((dict(), False), (dict(top_k=64), False), (dict(top_k=65), True), (dict(top_p=0.9), True),
                          (dict(top_k=3, top_p=0.5), True), (dict(top_p=1.0), False)):
        s2s = _stub_facade(4)
        s2s.sample_lines(LINES, n=2, temperature=0.5, seed=99, **kw)
        calls = s2s.engine.calls
        assert len(calls) == 3 and all(c.get('cut_entry', False) == cut_entry for c in calls), kw
        assert all(c['top_k'] == kw.get('top_k', 0) and c['tau'] == 0.5 and c['seed'] == 99 and c['N'] == 2 for c in calls), kw
        if cut_entry:
            assert all(c['top_p'] == kw.get('top_p', 1.0) and isinstance(c['top_p'], float) for c in calls), kw
    # (the plain stub of tests/test_sample_cases.py has no decode_sample_cut and no top_p keyword: the default call still runs on it)
    from tests.test_sample_cases import _stub_facade as plain
    assert plain(4).sample_lines(LINES, n=1, seed=1)[0][0]
    for bad in (0.0, -0.5, 1.5, float('nan'), None, 'much'):
        s2s = _stub_facade(4)
        with pytest.raises(ValueError, match='top_p'):
            s2s.sample_lines(LINES, top_p=bad)
        assert not s2s.engine.calls


# ------------------------------------------------------------------------------------------------------------------ 4. train()
def test_check_sampling_refuses_a_bad_cut():
    from cor_asv_ann_amd import training
    training.check_sampling('linear', 'sample', 1, 1.0, None)                      # (the five arguments of before)
    training.check_sampling('linear', 'sample', 1, 1.0, None, 5, 0.9)
    training.check_sampling('linear', 'greedy', 1, 1.0, None, 0, 1.0)
    for k, p, match in ((-1, 1.0, 'top_k'), (4096, 1.0, 'top_k'), (1.5, 1.0, 'top_k'), ('a', 1.0, 'top_k'), (0, 0.0, 'top_p'), (0, 1.5, 'top_p'),
                        (0, float('nan'), 'top_p'), (0, None, 'top_p')):
        with pytest.raises(ValueError, match=match):
            training.check_sampling('linear', 'sample', 1, 1.0, None, k, p)
    for k, p in ((5, 1.0), (0, 0.9)):
        with pytest.raises(ValueError, match='greedy'):
            training.check_sampling('linear', 'greedy', 1, 1.0, None, k, p)


def test_a_cut_joins_the_checkpoint_only_when_set(tmp_path, monkeypatch):
    from cor_asv_ann_amd import keras_h5
    from tests.test_sched_cases import _corpus, _model
    monkeypatch.chdir(tmp_path)
    corpus = _corpus(tmp_path)
    for kw in (dict(sample_top_p=0.9), dict(sample_schedule=0.5, sample_top_k=5), dict(sample_schedule=0.5, sample_pick='sample', sample_top_p=0.0)):
        s2s = _model(monkeypatch)
        with pytest.raises(ValueError, match='sample_top'):
            s2s.train([corpus], **kw)
        assert not s2s._stub, kw
    good = dict(sample_schedule=0.5, sample_pick='sample', sample_top_k=7, sample_top_p=0.9)
    first = _model(monkeypatch, epochs=2)
    first.train([corpus], **good)
    sampled = first._stub['e'].sampled
    assert sampled and all(k['top_k'] == 7 and k['top_p'] == 0.9 for k in sampled)
    (ck,) = glob.glob('model.ckpt.weights-01-*.h5')
    state = keras_h5.read_training_state(ck)['sample']
    assert state == dict(seed=sampled[0]['seed'], schedule='const:0.5', pick='sample', passes=1, temperature=1.0, top_k=7, top_p=0.9)
    for change, match in ((dict(sample_top_p=0.8), 'top_p differs'), (dict(sample_top_k=0), 'top_k differs'),
                          (dict(sample_top_k=0, sample_top_p=1.0), 'top_k differs')):
        with pytest.raises(ValueError, match=match):
            _model(monkeypatch, epochs=2).train([corpus], resume=ck, **dict(good, **change))
    resumed = _model(monkeypatch, epochs=2)
    resumed.train([corpus], resume=ck, **good)
    assert resumed._stub['e'].sampled and all(k['top_k'] == 7 and k['top_p'] == 0.9 for k in resumed._stub['e'].sampled)
    # without a cut: the keywords and the recorded settings of before
    for f in glob.glob('model.ckpt.*'):
        os.remove(f)
    plain = _model(monkeypatch, epochs=2)
    plain.train([corpus], sample_schedule=0.5, sample_pick='sample')
    assert all('top_k' not in k and 'top_p' not in k for k in plain._stub['e'].sampled)
    (ck,) = glob.glob('model.ckpt.weights-01-*.h5')
    assert sorted(keras_h5.read_training_state(ck)['sample']) == ['passes', 'pick', 'schedule', 'seed', 'temperature']
    with pytest.raises(ValueError, match='top_k differs'):         # (the first of the two recorded keys the file lacks)
        _model(monkeypatch, epochs=2).train([corpus], resume=ck, sample_schedule=0.5, sample_pick='sample', sample_top_p=0.9)


# ------------------------------------------------------------------------------------------------------------------ 5. the ABI
def test_the_four_entries_are_bound():
    import ctypes
    from cor_asv_ann_amd import _native as nv
    from cor_asv_ann_amd.engine import HipEngine
    sig = nv.SIGNATURES
    assert len(sig['casv_decode_sample_cut'][1]) == len(sig['casv_decode_sample'][1]) + 1 == 10
    assert len(sig['casv_debug_sample_cut_rows'][1]) == len(sig['casv_debug_sample_rows'][1]) + 1 == 15
    assert len(sig['casv_train_step_sampled_cut'][1]) == len(sig['casv_train_step_sampled'][1]) + 1 == 19
    assert len(sig['casv_debug_sched_cut_rows'][1]) == len(sig['casv_debug_sched_rows'][1]) + 1 == 11
    assert [f[0] for f in nv.SampleCut._fields_] == ['top_k', 'top_p'] and ctypes.sizeof(nv.SampleCut) == 8
    assert [f[0] for f in nv.SampleParams._fields_] == ['seed', 'temperature', 'top_k', 'samples']
    for name in ('decode_sample_cut', 'debug_sample_cut_rows', 'debug_sched_cut_rows'):
        assert callable(getattr(HipEngine, name))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'cor_asv_ann_hip.h')) as f:
        header = f.read()
    assert 'int32_t top_k;\n    float top_p;\n} casv_sample_cut;' in header
    assert 'int casv_decode_sample_cut(casv_model* m, const casv_sample_params* p, const casv_sample_cut* cut, int32_t S, const int64_t* stream,' in header
    assert 'int casv_debug_sample_cut_rows(casv_model* m, int32_t R, int32_t V, const casv_sample_params* p, const casv_sample_cut* cut,' in header
    assert 'int casv_train_step_sampled_cut(casv_model* m, int32_t mode, int32_t B, int32_t T, int32_t U, int32_t A,' in header
    assert 'int casv_debug_sched_cut_rows(casv_model* m, int32_t R, int32_t V, const casv_sched_params* p, const casv_sample_cut* cut,' in header
    csrc = os.path.join(root, 'cor_asv_ann_amd', 'csrc')
    with open(os.path.join(csrc, 'sample_row.h')) as f:
        row = f.read()
    assert 'sample_row_bound(' in row and 'sample_row_draw_under(' in row and 'sample_row_cut_bound(' in row
    for name, kernel in (('sample_kernels.hip', 'sample_cut_kernel'), ('sched_kernels.hip', 'sched_mix_cut_kernel')):
        with open(os.path.join(csrc, name)) as f:
            text = f.read()
        assert kernel in text and '#include "sample_row.h"' in text
