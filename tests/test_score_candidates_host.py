"""Without a GPU: the references of tests/candidate_cases.py leave nothing out of the GPU test's comparison, the facade's
score_candidates chunks, pads and files its results as documented (a stub engine records the calls), and the C header documents the
entry point _native binds."""
import os
import re

import numpy as np
import pytest

from tests import candidate_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ 1. the references
@pytest.mark.parametrize('c', cc.CASES, ids=cc.IDS)
def test_the_oracles_agree_everywhere(c):
    """best / rank are compared where the fp32 and the fp64 oracle agree (tests/test_gpu_score_candidates.py asks for a share of at
    least 0.98): here the share is 1, so the condition excludes nothing; and the case has the layout the table promises."""
    d, W, V, Be, N, L, flags, conf = c
    k = cc.case(c)
    o = cc.oracles(c)
    assert o['agree'].mean() == 1.0
    assert k['din'].shape == k['dout'].shape == (Be, N, L + 4) and k['enc_idx'].shape[:2] == (Be, L + 1)
    assert (k['enc_idx'].ndim == 3) == conf and (k['enc_val'] is not None) == conf
    flat = k['dout'].reshape(Be * N, -1)
    if N >= 2:
        assert (flat[-1] == -1).all() and (k['din'].reshape(Be * N, -1)[-1] == -1).all() and (k['wts'][-1] == 0).all()
        assert (flat[:-1] >= 0).any(axis=1).all()
    if Be * N > 1:
        assert (flat[1] >= 0).sum() == L // 2 + 1
    assert (flat[0] >= 0).sum() == L + 3                    # (a whole candidate: L + 2 characters and the newline)
    scored = flat >= 0
    print('%s: smallest target probability %.2e' % (cc.case_id(c), o['pt64'][scored].min()))
    assert o['pt64'][scored].min() > 1e-6                   # (the bounds' 2e-6 / p terms stay of the order of the results)
    assert np.array_equal(k['rep_idx'], np.repeat(k['enc_idx'], N, axis=0))


def test_the_table_reaches_what_it_names():
    rows = {(c[0], c[1], c[3], c[4]) for c in cc.CASES}
    assert (1, 32, 1, 1) in rows and any(c[0] == 1 and c[4] > 1 for c in cc.CASES)
    assert any(c[3] <= 32 < c[3] * c[4] for c in cc.CASES)                                  # decoder crosses a row block, encoder does not
    assert any(c[3] > 32 and (c[3] * c[4] + 31) // 32 > (c[3] + 31) // 32 for c in cc.CASES)    # both several, unequal
    assert any(c[1] == 512 for c in cc.CASES) and any(c[1] == 256 for c in cc.CASES) and any(c[1] % 32 for c in cc.CASES)
    assert any('bridge_dense' in c[6] for c in cc.CASES) and any('deep_bidirectional_encoder' in c[6] for c in cc.CASES)
    assert any(c[7] for c in cc.CASES) and len(cc.PLAIN) >= 8


# ------------------------------------------------------------------------------------------------------------------ 2. the facade
class _StubEngine:
    """Records every score_candidates call and answers arrays of the right shape whose entries name their place: logp[b, n, u] =
    -(the call's number + (code of dec_out[b, n, u]) / 1000)."""
    window_width = 5

    def __init__(self):
        self.calls = []

    def score_candidates(self, enc_idx, enc_val, dec_in, dec_out, want_align=False):
        B, T = enc_idx.shape[:2]
        assert dec_in.shape == dec_out.shape and dec_in.ndim == 3 and dec_in.shape[0] == B
        _, N, U = dec_in.shape
        self.calls.append(dict(enc_idx=enc_idx.copy(), dec_in=dec_in.copy(), dec_out=dec_out.copy(), want_align=want_align))
        k = len(self.calls)
        scored = dec_out >= 0
        logp = np.where(scored, -(k + dec_out / 1000.0), 0.0).astype(np.float32)
        best = np.where(scored, dec_out, 1).astype(np.int32)
        rank = np.where(scored, 0, -1).astype(np.int32)
        count = scored.sum(axis=2).astype(np.int32)
        nll = -logp.astype(np.float64).sum(axis=2)
        align = None
        if want_align == 'sparse':
            align = (np.zeros((B, N, U), np.int32), np.ones((B, N, U, 11), np.float32))
        elif want_align:
            align = np.broadcast_to(np.arange(B * N, dtype=np.float32).reshape(B, N, 1, 1), (B, N, U, T)).copy()
        return logp, best, rank, nll, count, align


def _facade(monkeypatch, batch_size):
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence
    from cor_asv_ann_amd.synthetic import make_vocabulary
    s2s = Sequence2Sequence()
    s2s.depth, s2s.width, s2s.voc_size, s2s.batch_size = 2, 32, 40, batch_size
    s2s.mapping = make_vocabulary(40)
    s2s.status = 2
    eng = _StubEngine()
    monkeypatch.setattr(s2s, '_require_engine', lambda: eng)
    return s2s, eng


def _lines(n, length, seed):
    from cor_asv_ann_amd.synthetic import make_lines
    return make_lines(n, length, seed, voc_size=40)[0]


def test_facade_chunks_pads_and_files_results(monkeypatch):
    s2s, eng = _facade(monkeypatch, batch_size=8)
    counts = [3, 2, 0, 4, 9, 1, 1, 2, 3]                    # candidates per source; source 6 is empty, source 4 has more than batch_size
    sources = _lines(len(counts), 7, 11)
    sources[6] = ''
    pool = _lines(sum(counts), 9, 12)
    candidates, at = [], 0
    for n in counts:
        candidates.append(pool[at:at + n]); at += n
    candidates[0][1] = ''                                   # an empty candidate among live ones
    candidates[3][2] = candidates[3][2][:3] + '\n'
    logprobs, scores, predictions, ranks, aligns = s2s.score_candidates(sources, candidates)
    # the shape of the answer: per source, per candidate, in input order
    for res in (logprobs, scores, predictions, ranks, aligns):
        assert [len(x) for x in res] == counts
    assert logprobs[2] == [] and scores[2] == [] and aligns[2] == []
    skipped = ([], 0.0, '', [], [])
    assert tuple(r[0][1] for r in (logprobs, scores, predictions, ranks, aligns)) == skipped
    assert tuple(r[6][0] for r in (logprobs, scores, predictions, ranks, aligns)) == skipped
    # the chunks: live sources 0 (2 live candidates), 1 (2), 3 (4), 4 (9), 5 (1), 7 (2), 8 (3) under a budget of 8 rows
    #   [0, 1] N = 2 (a third source would make 3 x 4 = 12 > 8) | [3] N = 4 (with source 4: 2 x 9 > 9) | [4] alone, N = 9 > batch_size
    #   | [5, 7] N = 2 (with source 8: 3 x 3 = 9 > 8) | [8] N = 3
    got = [(c['enc_idx'].shape[0], c['dec_out'].shape[1]) for c in eng.calls]
    assert got == [(2, 2), (1, 4), (1, 9), (2, 2), (1, 3)]
    for c in eng.calls:
        B, N, U = c['dec_out'].shape
        assert B * N <= max(8, N)                           # the row budget
        lens = (c['dec_out'] >= 0).sum(axis=2)
        assert lens.max() == U - 1 and c['enc_idx'].shape[1] == 8        # the chunk's padded lengths
        assert ((c['dec_out'] >= 0) == (np.arange(U)[None, None, :] < lens[:, :, None])).all()
        pad = lens == 0
        assert (c['dec_in'][pad] == -1).all() and (c['dec_out'][pad] == -1).all()         # padding candidates: all -1
        assert (c['dec_in'][~pad][:, 0] == -1).all() and np.array_equal(c['dec_in'][:, :, 1:][c['dec_out'][:, :, :-1] >= 0],
                                                                       c['dec_out'][:, :, :-1][c['dec_out'][:, :, :-1] >= 0])
        assert not c['want_align']
    assert [int((c['dec_out'] >= 0).any(axis=2).sum()) for c in eng.calls] == [4, 4, 9, 3, 3]
    pads = [(~(c['dec_out'] >= 0).any(axis=2)).tolist() for c in eng.calls]
    assert pads[3] == [[False, True], [False, False]]       # source 5 has one candidate of the chunk's two: the second is padding
    # results land at their source and candidate: the stub's logp names the call and the character
    chunk_of = {0: 1, 1: 1, 3: 2, 4: 3, 5: 4, 7: 4, 8: 5}
    for j, k in chunk_of.items():
        for i, line in enumerate(candidates[j]):
            if not line:
                continue
            codes = [s2s.mapping[0][ch] for ch in line]
            assert len(logprobs[j][i]) == len(line) == len(ranks[j][i])
            assert np.allclose(logprobs[j][i], [-(k + v / 1000.0) for v in codes], rtol=0, atol=1e-5)
            assert predictions[j][i] == line and ranks[j][i] == [0] * len(line)
            assert abs(scores[j][i] - np.mean([k + v / 1000.0 for v in codes])) < 1e-5
    # the source order inside a chunk is the input order
    assert np.array_equal(eng.calls[0]['enc_idx'][:, :7, 0], np.array([[s2s.mapping[0][ch] for ch in sources[j][:7]] for j in (0, 1)]))


def test_facade_alignment_forms_and_edge_inputs(monkeypatch):
    from cor_asv_ann_amd.realign import SparseAlignment
    s2s, eng = _facade(monkeypatch, batch_size=4)
    assert s2s.score_candidates([], []) == ([], [], [], [], [])
    assert s2s.score_candidates(['', _lines(1, 5, 3)[0]], [_lines(2, 5, 4), []]) == ([[[], []], []], [[0.0, 0.0], []], [['', ''], []],
                                                                                  [[[], []], []], [[[], []], []])
    assert eng.calls == []                                  # nothing to score: no call
    sources, pool = _lines(2, 6, 5), _lines(5, 8, 6)
    pool[4] = pool[4][:2] + '\n'
    candidates = [pool[:2], pool[2:]]
    dense = s2s.score_candidates(sources, candidates, alignments='dense')[4]
    assert eng.calls[-1]['want_align'] is True and len(eng.calls) == 2      # 2 x 3 = 6 > 4: one source per chunk
    for j in range(2):
        for i, line in enumerate(candidates[j]):
            rows = np.asarray(dense[j][i])
            assert rows.shape == (len(line), 7) and (rows == i).all()       # (the stub's rows hold b * N + n; one source per chunk: n)
    sparse = s2s.score_candidates(sources, candidates, alignments=True)[4]
    assert eng.calls[-1]['want_align'] == 'sparse'
    assert all(isinstance(sparse[j][i], SparseAlignment) and len(sparse[j][i]) == len(candidates[j][i])
               for j in range(2) for i in range(len(candidates[j])))
    with pytest.raises(AssertionError):
        s2s.score_candidates(sources, candidates[:1])


# ------------------------------------------------------------------------------------------------------------------ 3. the interface
def test_the_header_documents_the_entry_point_and_native_binds_it():
    from cor_asv_ann_amd import _native as nv
    with open(os.path.join(ROOT, 'include', 'cor_asv_ann_hip.h')) as f:
        text = f.read()
    m = re.search(r'/\*((?:[^*]|\*(?!/))*)\*/\s*int casv_score_candidates\(casv_model\* m, int32_t B, int32_t N, int32_t T, int32_t U, '
                  r'int32_t A,\s*const int32_t\* enc_idx, const float\* enc_val, const int32_t\* dec_in, const int32_t\* dec_out,\s*'
                  r'float\* logp, int32_t\* best, int32_t\* rank, double\* nll, int32_t\* count, float\* align\);', text)
    assert m
    doc = m.group(1)
    for word in ('kt:407', 's2s:491-497', '(B,N,U)', '(B,N,U,T)', 'all -1', 'N < 1', 'CASV_ERR_ARG', 'casv_score_get_alignments_sparse'):
        assert word in doc, word
    restype, argtypes = nv.SIGNATURES['casv_score_candidates']
    assert len(argtypes) == 16 and argtypes[1:6] == [nv.c_int32] * 5 and argtypes[6:] == [nv.c_void_p] * 10
    assert len(argtypes) == len(nv.SIGNATURES['casv_score_targets'][1]) + 1
    with open(os.path.join(ROOT, 'cor_asv_ann_amd', 'csrc', 'score.hip')) as f:
        train = f.read()
    assert 'extern "C" int casv_score_candidates(' in train
    # one path: both entry points are one call of the same function, casv_score_targets with N = 1
    for name, n in (('casv_score_targets', '1'), ('casv_score_candidates', 'N')):
        body = train[train.index('extern "C" int %s(' % name):]
        body = body[:body.index('\n}')]
        assert 'return score_call(m, B, %s, T, U, A, ' % n in body and body.count(';') == 1, name
