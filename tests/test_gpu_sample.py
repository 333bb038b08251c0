"""Sampling on the device (csrc/sample_kernels.hip: sample_kernel; csrc/decode.hip: casv_decode_sample; csrc/debug_rows.hip: casv_debug_sample_rows;
DESIGN.md section 4.8): the kernel alone against the float64 restatement and the scoring head's bits, the model against the oracle
forced along the device's own sequence, a row's bits whatever the batch, the edges and errors, and the facade.  Cases, references and
bounds: tests/sample_cases.py, held on the CPU by tests/test_sample_cases.py.  Runs with and without CASV_POISON=1."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

os.environ.setdefault('CASV_POISON', '1')      # read once by the library, at its first allocation

from tests import sample_cases as sa
from tests import score_cases as sc
from tests.decode_noise_cases import C_MAX


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same(a, b):
    """Bit for bit."""
    return all(np.array_equal(np.ascontiguousarray(x).view(np.int32), np.ascontiguousarray(y).view(np.int32)) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------------ a. the kernel alone
@pytest.fixture(scope='module')
def head_engine():
    from cor_asv_ann_amd.engine import HipEngine
    eng = HipEngine(1, 32, 40)
    yield eng
    eng.close()


def _check_rows(eng, x, tau, top_k, name, u=None, streams=None, samples=None, step=0, seed=0, pads=sc.PADS):
    """One batch of rows under the padding values: the pick where it is not left out, the head's bits, logq, the feedback rows."""
    R, V = x.shape
    s_ = np.arange(R) if streams is None else streams
    n_ = np.zeros(R, np.int64) if samples is None else samples
    uu = sa.uniform(seed, s_, n_, step) if u is None else np.asarray(u, np.float32)
    d64, d32 = sa.draw_rows(x, uu, tau, top_k), sa.draw_rows(x, uu, tau, top_k, np.float32)
    lo, _ = sa.left_out(uu, d64, d32)
    first = None
    for pad in pads:
        got = eng.debug_sample_rows(x, tau, top_k, seed=seed, step=step, streams=streams, samples=samples, u=u, pad_value=pad)
        first = first or got
        assert _same(got, first), (name, pad)                # no output bit moves with the padding columns
    idx, logp, logq, fb = first
    valid = d64['valid']
    assert np.array_equal(idx[valid & ~lo], d64['idx'][valid & ~lo]), (name, idx, d64['idx'], lo)
    assert (idx[~valid] == 1).all() and np.isnan(logp[~valid]).all() and np.isnan(logq[~valid]).all(), name
    rows = np.nonzero(valid)[0]
    assert d64['cand'][rows, idx[rows]].all() and (x[rows, idx[rows]] > -np.inf).all(), name        # (left out or not)
    # ... and left out or not, u lies within delta of the drawn index's own interval of the float64 CDF (at V = 4096 the boundaries
    # are closer than 2 delta: nearly every draw is left out of the exact comparison, none of this one)
    delta = np.maximum(C_MAX * np.abs(d32['cdf'] - d64['cdf']).max(axis=1), sa.OLD_RT)[rows]
    upper = d64['cdf'][rows, idx[rows]]
    lower = upper - d64['w'][rows, idx[rows]] / d64['w'][rows].sum(axis=1)
    assert (uu[rows] >= lower - delta).all() and ((uu[rows] <= upper + delta) | (upper >= 1 - 1e-12)).all(), name
    assert np.array_equal(_bits(fb), _bits(sa.onehot_rows(idx, valid, V))), name       # exactly one-hot: Vp - 1 exact zeros
    head = eng.debug_score_rows(x, idx)[0]                  # logp: the bits of the scoring head for that index as target
    finite = valid & np.isfinite(x.max(axis=1))
    assert np.array_equal(_bits(head[finite]), _bits(logp[finite])) and np.isnan(logp[valid & ~finite]).all(), name
    with np.errstate(divide='ignore', invalid='ignore'):    # logq of the index the device drew, in float64
        want = np.log(d64['w'][rows, idx[rows]] / d64['w'][rows].sum(axis=1))
    worst = float(sc.units_or_inf(logq[rows], want).max(initial=0.0)) / (4 * sc.e_np())
    print('%s: %d rows, %d left out, logq %.3f of the bound' % (name, R, int(lo.sum()), worst))
    assert worst <= 1, name
    return idx, lo


@pytest.mark.parametrize('c', sa.KERNEL_CASES, ids=['V%d_R%d_k%d_t%g' % c[:4] for c in sa.KERNEL_CASES])
def test_kernel_against_float64_and_the_head(head_engine, c):
    """With u = NULL: the picks are those of the reference's own Philox uniforms (the device's generator is pinned through its
    effects); the same rows with the uniforms handed in give the same bits."""
    V, R, top_k, tau, _ = c
    x, streams, samples, step, seed = sa.kernel_case(c)
    idx, lo = _check_rows(head_engine, x, tau, top_k, str(c), streams=streams, samples=samples, step=step, seed=seed)
    u = sa.uniform(seed, streams, samples, step)
    given = head_engine.debug_sample_rows(x, tau, top_k, u=u)
    assert _same(given, head_engine.debug_sample_rows(x, tau, top_k, seed=seed, step=step, streams=streams, samples=samples))
    # defaults: stream = the row's number, sample 0
    d = head_engine.debug_sample_rows(x, tau, top_k, seed=seed, step=step)
    assert _same(d, head_engine.debug_sample_rows(x, tau, top_k, u=sa.uniform(seed, np.arange(R), 0, step)))


def test_kernel_on_constructed_rows(head_engine):
    """Ties at the k-th place, -inf members, only index 0 finite, NaN, +inf, all equal: over a sweep of uniforms, u = 0 and
    u = 1 - 2^-24 among them."""
    u = np.concatenate([np.array([0.0, 1 - 2.0 ** -24]), (np.arange(30) + 0.5) / 30]).astype(np.float32)
    for name, x, top_k, tau, facts in sa.constructed_rows():
        if name == 'cold':
            u_ = u[1:]                  # (u = 0 on weights below float32's range: float64 still sees them)
        else:
            u_ = u
        rows = np.repeat(x[None], len(u_), axis=0)
        idx, lo = _check_rows(head_engine, rows, tau, top_k, name, u=u_)
        if facts['valid']:
            assert not lo[:2].any() or name == 'cold', name          # the two edges are compared
            if 'only' in facts:
                assert set(idx.tolist()) <= set(facts['only']), name
            assert 0 not in idx


@pytest.mark.parametrize('V,top_k,tau', [(12, 0, 1.0), (40, 5, 0.5), (96, 0, 2.0)])
def test_kernel_at_the_neighbours_of_every_boundary(head_engine, V, top_k, tau):
    """For each interior boundary of the float64 CDF the two float32 uniforms next to it OUTSIDE delta: the pick changes there and
    nowhere else."""
    rng = np.random.default_rng(V)
    x = (rng.standard_normal(V) * 1.5).astype(np.float32)
    probe = sa.draw_rows(x[None], [0.5], tau, top_k)
    d32 = sa.draw_rows(x[None], [0.5], tau, top_k, np.float32)
    c = probe['cdf'][0]
    bounds = np.unique(c[probe['cand'][0] & (c > 0) & (c < 1)])
    delta = max(C_MAX * float(np.abs(d32['cdf'] - probe['cdf']).max()), sa.OLD_RT)
    below = np.nextafter((bounds - delta).astype(np.float32), np.float32(-1))
    above = np.nextafter((bounds + delta).astype(np.float32), np.float32(2))
    u = np.concatenate([below, above])
    u = u[(u >= 0) & (u < 1)]
    idx, lo = _check_rows(head_engine, np.repeat(x[None], len(u), axis=0), tau, top_k, 'boundaries V=%d' % V, u=u, pads=sc.PADS[:1])
    assert (~lo).sum() >= len(bounds), (V, int((~lo).sum()), len(bounds))          # (a neighbour may fall within delta of the NEXT boundary)


def test_kernel_arguments(head_engine):
    from cor_asv_ann_amd._native import NativeError
    x = np.zeros((2, 40), np.float32)
    for kw in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=np.inf), dict(temperature=np.nan), dict(top_k=-1),
               dict(top_k=65), dict(step=-1), dict(step=2 * 4096)):
        with pytest.raises(NativeError) as e:
            head_engine.debug_sample_rows(x, **kw)
        assert e.value.code == -1, kw
        assert any(word in str(e.value) for word in ('temperature', 'top_k', 'step')), str(e.value)
    with pytest.raises(NativeError) as e:
        head_engine.debug_sample_rows(np.zeros((1, 4097), np.float32))
    assert e.value.code == -1


def test_kernel_is_timed_under_its_own_class(head_engine):
    head_engine.profile(True)
    before = head_engine.profile_read('sample')['launches']
    head_engine.debug_sample_rows(np.zeros((5, 40), np.float32))
    assert head_engine.profile_read('sample')['launches'] == before + 1
    head_engine.profile(False)


# ------------------------------------------------------------------------------------------------------------------ b. the model
def _engine(case, arithmetic=None):
    from cor_asv_ann_amd.engine import HipEngine
    mc = sa.build_model(case)
    eng = HipEngine(case[1], case[2], case[3], **mc['flags'])
    eng.set_weights(mc['w'])
    if arithmetic is not None:
        eng.set_option('arithmetic', arithmetic)
    return eng, mc


@pytest.mark.parametrize('arithmetic', (0, 2))
@pytest.mark.parametrize('case', sa.MODEL_CASES, ids=sa.MODEL_IDS)
def test_samples_match_the_oracle_forced_along_them(case, arithmetic):
    """Measured on an MI355X (profiles/sample_noise.txt): see there for the figures of every case."""
    eng, mc = _engine(case, arithmetic)
    N, seed = mc['N'], 4242
    try:
        eng.encode(mc['idx'], mc['val'])
        for tau, top_k in sa.DRAWS:
            got = eng.decode_sample(N, tau, top_k, seed, want_align=True)
            again = eng.decode_sample(N, tau, top_k, seed, want_align='sparse')
            assert _same(got[:4], again[:4])
            f = sa.check_model(case, got, tau, top_k, seed, align=got[4], sparse=again[4])
            print('%s arithmetic %d tau=%g k=%d: %d draws, %d left out, %d wrong, smallest delta that matches every draw %.3g; exp(logp) '
                  '(rms, max) = (%.3f, %.3f), alignment rows (%.3f, %.3f), sparse (%.3f, %.3f) units; logq off by %.3g'
                  % ((case[0], arithmetic, tau, top_k, f['draws'], f['left_out'], f['wrong'], f['need']) + f['logp'] + f['align'] + f['sparse'] + (f['logq'],)))
            assert f['wrong'] == 0
            assert f['left_out'] <= sa.LEFT_OUT_CAP * f['draws']
            assert f['logp'][1] <= C_MAX and f['align'][1] <= C_MAX and f['sparse'][1] <= C_MAX
            if (tau, top_k) == (1.0, 1):        # the reference's argmax-with-one-hot-feedback run, up to a row's first left-out draw
                B, S = mc['x'].shape[0], got[0].shape[2]
                _, _, greedy = sa.forced(case, np.zeros((B, N, S)), np.float64, lambda s, p: 1 + p[:, 1:].argmax(axis=1))
                lo = sa.left_out_mask(f['ref'], tau, top_k)
                seq = got[0].reshape(B * N, S)
                for r in range(B * N):
                    n = int(got[3].reshape(-1)[r])
                    if lo[r, :n].any():
                        n = int(np.argmax(lo[r, :n]))
                    assert np.array_equal(seq[r, :n], greedy[r, :n]), (case[0], r)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------ c. never by the batch
def _reported(got, b, n):
    """(idx, logp bits, logq bits) of the reported steps of row (b, n)."""
    k = int(got[3][b, n])
    return got[0][b, n, :k].tolist(), _bits(got[1][b, n, :k]).tolist(), _bits(got[2][b, n, :k]).tolist()


def test_a_row_never_depends_on_the_batch():
    case = sa.BATCH_CASE
    eng, mc = _engine(case)
    idx = mc['idx']
    B = len(idx)
    kw = dict(temperature=0.8, top_k=7, seed=99)
    try:
        eng.encode(idx)
        seven = eng.decode_sample(1, **kw)
        eng.encode(idx[3:4])
        alone = eng.decode_sample(1, streams=[3], **kw)
        assert _reported(alone, 0, 0) == _reported(seven, 3, 0)                     # alone, and as line 3 of 7
        eng.encode(idx)
        two, four = eng.decode_sample(2, **kw), eng.decode_sample(4, **kw)
        for b in range(B):
            assert _reported(two, b, 0) == _reported(four, b, 0) == _reported(seven, b, 0)
            assert _reported(two, b, 1) == _reported(four, b, 1)
        perm = np.array([4, 0, 6, 2, 5, 1, 3])
        eng.encode(idx[perm])
        moved = eng.decode_sample(2, streams=perm, **kw)
        for j, b in enumerate(perm):
            for n in range(2):
                assert _reported(moved, j, n) == _reported(two, b, n)
        eng.encode(idx)
        assert _same(eng.decode_sample(2, **kw)[:4], two[:4])                       # the same seed: the same call
        other = eng.decode_sample(2, **dict(kw, seed=100))
        assert not np.array_equal(other[0], two[0])                                  # another seed: other lines somewhere
        streams = eng.decode_sample(2, streams=np.arange(B) + 2 ** 32, **kw)
        assert not np.array_equal(streams[0], two[0])                                # ... and other streams
        rows = [_reported(two, b, n)[0] for b in range(B) for n in range(2)]
        assert len(set(map(tuple, rows))) > B                                        # the samples of a line are not copies
    finally:
        eng.close()


def test_other_entry_points_are_untouched_by_a_sample_call():
    case = sa.BATCH_CASE
    eng, mc = _engine(case)
    idx = mc['idx']
    din = np.where(idx >= 0, np.roll(idx, 1, axis=1), -1).astype(np.int32)
    din[:, 0] = -1

    def others():
        eng.encode(idx)
        g = eng.decode_greedy(mode=0, want_align=True)
        b = eng.decode_beam(batch_size=4, max_results=2, want_align=True)
        s = eng.score_targets(idx, None, din, idx)
        return g, [b[k] for k in ('idx', 'prob', 'len', 'score', 'rej', 'align', 'n_found')], s[:5]
    try:
        before = others()
        eng.encode(idx)
        eng.decode_sample(3, seed=1)
        after = others()
        for a, b in zip(before, after):
            for x, y in zip(a, b):
                assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()
        # a sample between an encode and a greedy decode of the SAME encoding
        eng.encode(idx)
        eng.decode_sample(3, seed=1)
        g = eng.decode_greedy(mode=0, want_align=True)
        for x, y in zip(before[0], g):
            assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------ d. edges and errors
def test_state_and_argument_errors():
    from cor_asv_ann_amd._native import NativeError
    from cor_asv_ann_amd import _native as nv
    case = sa.BATCH_CASE
    eng, mc = _engine(case)

    def refused(call, code, word=None):
        with pytest.raises(NativeError) as e:
            call()
        assert e.value.code == code and (word is None or word in str(e.value)), str(e.value)
    try:
        refused(lambda: eng.decode_sample(2, steps=4), -2, 'casv_encode')                  # sample before encode
        eng.encode(mc['idx'])
        first = eng.decode_sample(2, seed=3)
        refused(lambda: eng.decode_sample(0), -1, 'samples=0')
        refused(lambda: eng.decode_sample(-2), -1, 'samples=-2')
        for tau in (0.0, -0.5, np.inf, -np.inf, np.nan):
            refused(lambda: eng.decode_sample(2, temperature=tau), -1, 'temperature')
        refused(lambda: eng.decode_sample(2, top_k=-1), -1, 'top_k=-1')
        refused(lambda: eng.decode_sample(2, top_k=65), -1, 'top_k=65')
        refused(lambda: eng.decode_sample(2, steps=2 * 4096 + 1), -1, 'S=8193')
        B, S = eng.B, 4
        p = nv.SampleParams(1, 1.0, 0, 2)
        bufs = [np.empty((B * 2, S), np.int32), np.empty((B * 2, S), np.float32), np.empty((B * 2, S), np.float32), np.empty(B * 2, np.int32)]
        for k in range(4):                                                      # NULL outputs
            args = [nv.ptr(b) for b in bufs]
            args[k] = None
            refused(lambda: nv.check(eng.lib.casv_decode_sample(eng.handle, ctypes.byref(p), S, None, *(args + [None]))), -1, 'null')
        refused(lambda: nv.check(eng.lib.casv_decode_sample(eng.handle, None, S, None, *([nv.ptr(b) for b in bufs] + [None]))), -1, 'null')
        refused(lambda: nv.check(eng.lib.casv_decode_sample(eng.handle, ctypes.byref(p), 0, None, *([nv.ptr(b) for b in bufs] + [None]))), -1, 'S=0')
        assert _same(eng.decode_sample(2, seed=3)[:4], first[:4])               # a refused call changed nothing
        # the sparse alignments after sampling serve B * N rows
        dense = eng.decode_sample(2, seed=3, want_align=True)
        lo, w = eng.alignments_sparse(eng.B * 2, dense[0].shape[2])
        assert lo.shape == (eng.B * 2, dense[0].shape[2])
        for b in range(eng.B):
            for n in range(2):
                for s in range(int(dense[3][b, n])):
                    row = np.zeros(eng.T + w.shape[2], np.float32)
                    row[lo[b * 2 + n, s]:lo[b * 2 + n, s] + w.shape[2]] = w[b * 2 + n, s]
                    assert np.array_equal(_bits(row[:eng.T]), _bits(dense[4][b, n, s]))
    finally:
        eng.close()


def test_a_nan_row_ends_there_and_leaves_the_others_their_bits():
    """Line 1's encoder output is NaN at a position the attention window of one of its rows reaches only after the first step: that
    row reports index 1 and NaN there and ends, the call returns CASV_ERR_NAN with every output filled, the rows of the other lines
    keep their bits."""
    from cor_asv_ann_amd._native import NativeError, CASV_ERR_NAN
    case = sa.MODEL_CASES[1]
    eng, mc = _engine(case)
    N, S, kw = 2, 8, dict(seed=17, temperature=1.0, top_k=0)
    _, enc, states, _ = sa._encoded(case, np.float32)
    enc, states = np.array(enc, np.float32), [np.array(s, np.float32) for s in states[:-1]]
    try:
        eng.set_encoder_outputs(enc, states)
        clean = eng.decode_sample(N, steps=S, want_align=True, **kw)
        inside = clean[4][1] > 0                                            # (N, S, T): the windows of line 1's rows
        first = np.where(inside.any(axis=1), inside.argmax(axis=1), S)       # (N, T): the step a position is first attended at
        cand = [(first[:, q].min(), q) for q in range(inside.shape[2]) if 1 <= first[:, q].min() < S]
        assert cand, 'no position enters a window after the first step'
        cand.sort(key=lambda t: (t[0] != 2, t[0]))                           # step 2 if there is one
        at, q = cand[0]
        bad = enc.copy()
        bad[1, q] = np.nan
        eng.set_encoder_outputs(bad, states)
        with pytest.raises(NativeError) as e:
            eng.decode_sample(N, steps=S, want_align=True, **kw)
        assert e.value.code == CASV_ERR_NAN
        got = e.value.outputs
        for n in range(N):
            k = int(first[n, q])
            if k >= int(clean[3][1, n]):                                     # the row's line ended before it looked there
                assert _reported(got, 1, n) == _reported(clean, 1, n)
                continue
            assert got[3][1, n] == k + 1 and got[0][1, n, k] == 1 and np.isnan(got[1][1, n, k]) and np.isnan(got[2][1, n, k])
            assert got[0][1, n, :k].tolist() == clean[0][1, n, :k].tolist() and np.array_equal(_bits(got[1][1, n, :k]), _bits(clean[1][1, n, :k]))
        assert any(first[n, q] < clean[3][1, n] for n in range(N))
        for b in range(len(enc)):
            if b != 1:
                for n in range(N):
                    assert _reported(got, b, n) == _reported(clean, b, n)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------ e. the facade
def _facade(case, batch_size, seed=None):
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence
    from oracle.decode import OracleModel
    mc = sa.build_model(case)
    s2s = Sequence2Sequence()
    s2s.depth, s2s.width, s2s.batch_size = case[1], case[2], batch_size
    s2s.mapping, s2s.voc_size = OracleModel(mc['cfg'], mc['w']).mapping, case[3]
    s2s.seed = seed
    s2s.configure()
    s2s.set_weights(mc['w'])
    s2s.status = 2
    i_c = s2s.mapping[1]
    return s2s, [''.join(i_c[int(i)] for i in row) for row in mc['idx']]


def test_sample_lines_through_the_facade():
    case = sa.FACADE_CASE
    s2s, lines = _facade(case, 4)
    assert all(line.endswith('\n') and len(line) == len(lines[0]) for line in lines)
    n, seed, T = 2, 5, len(lines[0])
    sources = lines[:2] + [''] + lines[2:]
    cands, logps, scores, logqs, aligns = s2s.sample_lines(sources, n=n, seed=seed, alignments=True)
    assert cands[2] == logps[2] == scores[2] == logqs[2] == aligns[2] == []              # the empty source
    c_i = s2s.mapping[0]
    for j, line in enumerate(sources):
        if not line:
            continue
        assert len(cands[j]) == len(logps[j]) == len(scores[j]) == len(logqs[j]) == len(aligns[j]) == n
        for k in range(n):
            text = cands[j][k]
            assert isinstance(text, str) and len(text) == len(logps[j][k]) == len(logqs[j][k]) == len(aligns[j][k])
            assert text.endswith('\n') or len(text) == 2 * T                            # cut at S = 2T only
            assert '\n' not in text[:-1]
            assert scores[j][k] == pytest.approx(-np.sum(logps[j][k], dtype=np.float64) / len(text), rel=1e-12)
    # streams default to the index in the CALL: line j alone, under stream j, is the row it was in its chunk (batch_size 4, n = 2:
    # chunks of two sources, so sources 3 .. 6 sit at places 0 and 1 of theirs)
    for j in (1, 3, 4, 6):
        alone = s2s.sample_lines([sources[j]], n=n, seed=seed, streams=[j])
        assert alone[0][0] == cands[j] and alone[1][0] == logps[j] and alone[3][0] == logqs[j]
    wrong = s2s.sample_lines([sources[4]], n=n, seed=seed)                                 # (stream 0: another line)
    assert wrong[0][0] != cands[4]
    # score_candidates on the candidates: both against the oracle forced along them, within the bound of the model test
    live = [j for j, line in enumerate(sources) if line]
    rescored = s2s.score_candidates(sources, cands)[0]
    S = 2 * T
    seq = np.full((len(live), n, S), sa.EOS, np.int64)
    for b, j in enumerate(live):
        for k in range(n):
            seq[b, k, :len(cands[j][k])] = [c_i[ch] for ch in cands[j][k]]
    P64, _, _ = sa.forced(case, seq, np.float64)
    P32, _, _ = sa.forced(case, seq, np.float32)
    ours, theirs, p64, p32 = [], [], [], []
    for b, j in enumerate(live):
        for k in range(n):
            m = len(cands[j][k])
            assert len(rescored[j][k]) == m
            ours += logps[j][k]
            theirs += rescored[j][k]
            p64 += P64[b * n + k, np.arange(m), seq[b, k, :m]].tolist()
            p32 += P32[b * n + k, np.arange(m), seq[b, k, :m]].tolist()
    r_ours = sa.ratio(np.exp(np.array(ours, np.float64)), np.array(p32), np.array(p64), rel=True)
    r_theirs = sa.ratio(np.exp(np.array(theirs, np.float64)), np.array(p32), np.array(p64), rel=True)
    print('sample_lines logp (rms, max) = (%.3f, %.3f), score_candidates (%.3f, %.3f) units' % (r_ours + r_theirs))
    assert r_ours[1] <= C_MAX and r_theirs[1] <= C_MAX
    s2s.engine.close()


def test_seed_none_is_repeatable_under_self_seed():
    runs = []
    for _ in range(2):
        s2s, lines = _facade(sa.FACADE_CASE, 4, seed=7)
        a = s2s.sample_lines(lines[:3], n=2)
        b = s2s.sample_lines(lines[:3], n=2)
        runs.append((a[0], a[1], b[0], b[1]))
        s2s.engine.close()
    assert runs[0] == runs[1]
    assert runs[0][0] != runs[0][2]                 # two calls draw two seeds
