"""The references and bounds of tests/test_gpu_sample.py hold on the CPU: the generator gives the published known answers and is
uniform, the restated sampler keeps the rules on rows built by hand, the reference alone stays inside the ambiguity cap on the model
cases with o32 and o64 agreeing outside the margin, the facade's sample_lines keeps its books on a stub engine, and both entries
are bound."""
import numpy as np
import pytest

from tests import sample_cases as sa


# ------------------------------------------------------------------------------------------------------------------ 1. the generator
def test_philox_known_answers():
    for counter, key, want in sa.KNOWN_ANSWERS:
        got = tuple(int(x) for x in sa.philox4x32_10(counter, key))
        assert got == want, ['%08x' % x for x in got]


def _grid(seed=12345):
    return sa.uniform(seed, np.arange(64)[:, None, None], np.arange(8)[None, :, None], np.arange(32)[None, None, :])


def test_uniform_range_and_distinct_words():
    u = _grid()
    assert u.dtype == np.float32 and u.shape == (64, 8, 32)
    assert (u >= 0).all() and (u < 1).all()
    out = sa.philox4x32_10((np.arange(64)[:, None, None], 0, np.arange(8)[None, :, None], np.arange(32)[None, None, :]), (12345, 0))
    # distinct counters give distinct outputs: the rounds are a bijection of the 128-bit counter (a single 32-bit word of 16384
    # may repeat by chance, probability 3 %: it is the four words together that cannot)
    words = np.stack([np.broadcast_to(o, (64, 8, 32)) for o in out], axis=-1).reshape(-1, 4)
    assert len(np.unique(words, axis=0)) == len(words) == 16384
    assert np.array_equal(((words[:, 0] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32), u.ravel())
    # stream ids of 2^32 and more reach the second counter word; a seed of 2^32 and more the second key word
    assert not np.array_equal(sa.uniform(1, np.arange(64) + 2 ** 32, 0, 0), sa.uniform(1, np.arange(64), 0, 0))
    assert not np.array_equal(sa.uniform(1 + 2 ** 32, np.arange(64), 0, 0), sa.uniform(1, np.arange(64), 0, 0))
    assert not np.array_equal(sa.uniform(2, np.arange(64), 0, 0), sa.uniform(1, np.arange(64), 0, 0))


def test_uniform_moments():
    u = _grid().astype(np.float64).ravel()
    n = u.size
    assert abs(u.mean() - 0.5) <= 5 * np.sqrt(1.0 / 12 / n)               # sigma of the mean of n uniforms
    counts = np.histogram(u, bins=16, range=(0, 1))[0]
    sigma = np.sqrt(n * (1 / 16) * (15 / 16))                              # binomial
    assert (np.abs(counts - n / 16) <= 5 * sigma).all(), counts


# ------------------------------------------------------------------------------------------------------------------ 2. the rules
U_EDGES = (0.0, 1 - 2.0 ** -24)
U_SWEEP = np.concatenate([np.array(U_EDGES), (np.arange(97) + 0.5) / 97]).astype(np.float32)


def test_sampler_rules_on_constructed_rows():
    for name, x, top_k, tau, facts in sa.constructed_rows():
        V = len(x)
        d = sa.draw_rows(np.repeat(x[None], len(U_SWEEP), axis=0), U_SWEEP, tau, top_k)
        assert d['valid'].all() == facts['valid'] and d['valid'].any() == facts['valid'], name
        if not facts['valid']:
            assert (d['idx'] == 1).all() and np.isnan(d['logq']).all(), name
            continue
        drawn = set(d['idx'].tolist())
        assert 0 not in drawn and all(1 <= v < V for v in drawn), name
        assert np.isfinite(x[d['idx']]).all(), name                        # a -inf entry is never drawn
        if 'only' in facts:
            assert drawn == set(facts['only']), (name, drawn)
        for v in facts.get('never', ()):
            assert v not in drawn, name
        w = d['w'][0]
        positive = np.nonzero(w > 0)[0]
        assert d['idx'][0] == positive[0], name                            # u = 0: the first candidate with w > 0
        # u = 1 - 2^-24: the last candidate with w > 0 -- where its weight is more than the 2^-24 Z that u leaves above it
        # (every row but the cold one, whose tail weights are e^-1000 gaps)
        assert w[positive[-1]] > 2.0 ** -23 * w.sum() or name == 'cold', name
        if name != 'cold':
            assert d['idx'][1] == positive[-1], name
        assert np.allclose(np.exp(d['logq']), (w / w.sum())[d['idx']], rtol=1e-12), name
        if name == 'cold':              # tau = 1e-3: the argmax over 1 .. V-1 (but for u = 0 exactly, where float64 still sees e^-1000)
            assert set(d['idx'][1:].tolist()) == {1 + int(np.argmax(x[1:]))}


def test_float32_restatement_agrees_on_the_kernel_table():
    """The float32 restatement of the definition draws what the float64 one draws outside the margin, on every kernel case."""
    for c in sa.KERNEL_CASES:
        V, R, top_k, tau, _ = c
        x, streams, samples, step, seed = sa.kernel_case(c)
        u = sa.uniform(seed, streams, samples, step)
        d64, d32 = sa.draw_rows(x, u, tau, top_k), sa.draw_rows(x, u, tau, top_k, np.float32)
        lo, _ = sa.left_out(u, d64, d32)
        assert np.array_equal(d64['cand'], d32['cand'])
        assert np.array_equal(d64['idx'][~lo], d32['idx'][~lo]), c
        assert d64['cand'].sum(axis=1).tolist() == [min(top_k, V - 1) if top_k else V - 1] * R


# ------------------------------------------------------------------------------------------------------------------ 3. the cap
@pytest.mark.parametrize('case,tau,top_k', sa.CPU_CASES, ids=['%s_t%g_k%d' % (c[0], t, k) for c, t, k in sa.CPU_CASES])
def test_reference_stays_inside_the_ambiguity_cap(case, tau, top_k):
    ref = sa.reference_run(case, tau, top_k, seed=2024)
    seq = ref['seq']
    reported = np.arange(seq.shape[1])[None, :] < sa.lengths(seq)[:, None]
    n, out, wrong, disagree, need = sa.compare_draws(ref, seq, tau, top_k, reported)
    print('%s tau=%g k=%d: %d draws, %.1f %% left out, %d o32/o64 disagreements outside the margin' % (case[0], tau, top_k, n, 100.0 * out / n, disagree))
    assert n > 100 and out <= sa.LEFT_OUT_CAP * n
    assert wrong == 0 and disagree == 0 and need == 0.0                    # (the sequence IS the float64 pick)


def test_argmax_with_one_hot_feedback_is_top_k_1():
    case = sa.MODEL_CASES[0]
    ref = sa.reference_run(case, 1.0, 1, seed=7)
    B, N = sa.build_model(case)['x'].shape[0], case[6]
    _, _, greedy = sa.forced(case, np.zeros((B, N, ref['seq'].shape[1])), np.float64, lambda s, p: 1 + p[:, 1:].argmax(axis=1))
    assert np.array_equal(ref['seq'], greedy)
    assert (ref['seq'].reshape(B, N, -1) == ref['seq'].reshape(B, N, -1)[:, :1]).all()          # every sample of a line the same


# ------------------------------------------------------------------------------------------------------------------ 4. the facade
class _StubEngine(object):
    """encode / decode_sample with made-up values that encode (call, line, sample, step), and a record of the calls."""
    def __init__(self):
        self.calls = []

    def encode(self, idx, val=None, src_rej=None):
        self.B, self.T = idx.shape[:2]
        self.idx = idx.copy()

    def decode_sample(self, samples, temperature=1.0, top_k=0, seed=0, streams=None, steps=None, want_align=False):
        B, N, S = self.B, samples, 2 * self.T
        self.calls.append(dict(idx=self.idx, N=N, tau=temperature, top_k=top_k, seed=seed, streams=np.array(streams), want_align=want_align))
        gi = np.full((B, N, S), 5, np.int32)
        length = np.empty((B, N), np.int32)
        for b in range(B):
            for n in range(N):
                length[b, n] = min(1 + (int(streams[b]) + n) % 4, S)
                gi[b, n, length[b, n] - 1] = 1                              # the end-of-line
        gi[0, 0, :] = 5
        length[0, 0] = S                                                    # a row cut at S: no end-of-line
        k = len(self.calls) - 1
        lp = -(100.0 * k + 10.0 * np.arange(B)[:, None, None] + np.arange(N)[None, :, None] + 0.125 * np.arange(S)[None, None, :]).astype(np.float32)
        return gi, lp, lp - 1, length, None


def _stub_facade(batch_size, voc_size=100):
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence
    from oracle import make_vocabulary
    s2s = Sequence2Sequence()
    s2s.depth, s2s.width, s2s.batch_size = 1, 32, batch_size
    s2s.mapping, s2s.voc_size = make_vocabulary(voc_size), voc_size
    s2s.engine = _StubEngine()
    s2s._require_engine = lambda: s2s.engine
    s2s.status = 2
    return s2s


LINES = ['abc\n', 'def\n', '', 'ghi\n', 'jkl\n', 'mno\n', 'pqr\n']


def test_sample_lines_bookkeeping_on_a_stub_engine():
    s2s = _stub_facade(4)
    cands, logps, scores, logqs, aligns = s2s.sample_lines(LINES, n=2, temperature=0.5, top_k=3, seed=99)
    calls = s2s.engine.calls
    assert [c['streams'].tolist() for c in calls] == [[0, 1], [3, 4], [5, 6]]          # the index in the CALL, across the chunks
    assert all(c['N'] == 2 and c['tau'] == 0.5 and c['top_k'] == 3 and c['seed'] == 99 and c['want_align'] is False for c in calls)
    i_c = s2s.mapping[1]
    for j, line in enumerate(LINES):
        if not line:
            assert cands[j] == logps[j] == scores[j] == logqs[j] == aligns[j] == []
            continue
        assert len(cands[j]) == len(logps[j]) == len(scores[j]) == len(logqs[j]) == len(aligns[j]) == 2
        k, b = [(k, c['streams'].tolist().index(j)) for k, c in enumerate(calls) if j in c['streams']][0]
        for n in range(2):
            cut = (b, n) == (0, 0)                                      # (the stub's first row of every call)
            c = 8 if cut else 1 + (j + n) % 4
            assert cands[j][n] == i_c[5] * (c if cut else c - 1) + ('' if cut else '\n')
            want = [-(100.0 * k + 10.0 * b + n + 0.125 * s) for s in range(c)]
            assert logps[j][n] == want and logqs[j][n] == [x - 1 for x in want]
            assert scores[j][n] == pytest.approx(-sum(want) / c, rel=1e-12) and isinstance(scores[j][n], float)
            assert aligns[j][n] == []
    # a source with more samples than batch_size goes alone
    s2s = _stub_facade(4)
    s2s.sample_lines(LINES[:2], n=5, seed=1)
    assert [c['streams'].tolist() for c in s2s.engine.calls] == [[0], [1]]
    # streams handed in; seed=None: drawn from the generator self.seed seeds
    s2s = _stub_facade(8)
    s2s.sample_lines(LINES, n=2, seed=3, streams=[70, 71, 72, 73, 74, 75, 2 ** 40])
    assert [c['streams'].tolist() for c in s2s.engine.calls] == [[70, 71, 73, 74], [75, 2 ** 40]]
    seeds = []
    for _ in range(2):
        s2s = _stub_facade(8)
        s2s._rng = np.random.default_rng(11)
        s2s.sample_lines(LINES[:2], n=1)
        s2s.sample_lines(LINES[:2], n=1)
        seeds.append([c['seed'] for c in s2s.engine.calls])
    assert seeds[0] == seeds[1] and seeds[0][0] != seeds[0][1] and all(0 <= s < 2 ** 64 for s in seeds[0])
    assert s2s.sample_lines([]) == ([], [], [], [], [])
    with pytest.raises(ValueError):
        s2s.sample_lines(LINES, n=0)
    s2s.status = 1
    with pytest.raises(AssertionError):
        s2s.sample_lines(LINES)


def test_both_entries_are_bound():
    import os
    from cor_asv_ann_amd import _native as nv
    assert len(nv.SIGNATURES['casv_decode_sample'][1]) == 9 and len(nv.SIGNATURES['casv_debug_sample_rows'][1]) == 14
    assert [f[0] for f in nv.SampleParams._fields_] == ['seed', 'temperature', 'top_k', 'samples']
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'cor_asv_ann_hip.h')) as f:
        header = f.read()
    assert 'int casv_decode_sample(casv_model* m, const casv_sample_params* p, int32_t S, const int64_t* stream,' in header
    assert 'int casv_debug_sample_rows(casv_model* m, int32_t R, int32_t V, const casv_sample_params* p, int32_t step,' in header
    with open(os.path.join(root, 'cor_asv_ann_amd', 'csrc', 'Makefile')) as f:
        assert ' sample_kernels.hip ' in f.read()
    # the order the two kernels select by lives in one header
    csrc = os.path.join(root, 'cor_asv_ann_amd', 'csrc')
    for name in ('train_kernels.hip', 'sample_kernels.hip'):
        with open(os.path.join(csrc, name)) as f:
            text = f.read()
        assert '#include "alt_order.h"' in text and 'unsigned long long alt_key(' not in text
