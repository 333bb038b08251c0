"""The beam search's order rules on a real MI355X, on models with exact ties (tests/tie_models.py): casv_decode_beam against
oracle.decode.decode_sequence_beam for EVERY line and EVERY returned result -- no line is left out, since on these models the
result is decided by the bookkeeping rules and not by rounding (tests/test_tie_models.py shows that on the CPU, and that each
flipped rule changes an expected output).

Exact: n_found, n_steps, every result's characters, length and rejection positions, the most new keys of a step; probabilities
exact where they are fl32(1/V) or the rejection threshold, else rtol 2e-4 (the suite's tolerance for probabilities); scores rtol
2e-4; alignments rtol 2e-4 + atol 2e-6 with rejection steps exactly one-hot, the window form equal to the dense rows bit for bit.
Each case runs as each line alone, all lines in one batch and the lines reversed -- the three bit for bit --, under arithmetic 0
and 2, and the lm_predict subset with the option on against tests/lm_oracle.py.

Preconditions come first, so that a failure points at the search and not at the model: one casv_decoder_step on the model gives
identical probabilities for identical E rows, exactly fl32(1/V) on the uniform family, and on the held-state family the same bits
at step 2 as at step 1."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

os.environ.setdefault('CASV_POISON', '1')      # read once by the library, at its first allocation

from oracle.decode import decode_sequence_beam
from tests.lm_oracle import decode_sequence_beam_lm
from tests.tie_models import CASES, BY_NAME, groups_of, run_search
from tests.tie_models import bits as _bits, same_bits as _same_bits, against_the_oracle as _against_the_oracle

_oracle = {}


def _expected(case, lm):
    """Per line (results of the oracle, its stats, rejection positions per result, trace of tie_models.search)."""
    key = (case.name, lm)
    if key in _oracle:
        return _oracle[key]
    m = case.model()
    enc_in, idx = case.inputs(m)
    enc = m.encode(enc_in)
    traced = run_search(case, lm=lm)
    out = []
    for j in range(len(case.lines)):
        stats = {}
        res = list((decode_sequence_beam_lm if lm else decode_sequence_beam)(
            m, source_seq=enc_in[j], encoder_outputs=[e[j:j + 1] for e in enc], stats=stats))
        rej = [list(r[4]) for r in (res if lm else traced[j][0])]
        assert [r[0] for r in traced[j][0]] == [r[0] for r in res] and traced[j][1] == stats
        out.append((res, stats, rej, traced[j][2]))
    _oracle[key] = (m, idx, out)
    return _oracle[key]


def _engine(case, arithmetic, lm):
    from cor_asv_ann_amd.engine import HipEngine
    eng = HipEngine(case.cfg.depth, case.cfg.width, case.V)
    eng.set_weights(case.weights())
    eng.set_option('arithmetic', arithmetic)
    eng.set_option('lm_predict', int(lm))
    return eng


def _preconditions(eng, case, idx):
    B, T = idx.shape
    eng.encode(idx)
    _, states = eng.encoder_outputs()
    line = np.arange(B, dtype=np.int32)
    a0 = np.zeros((B, T), np.float32)
    p1, st1 = eng.decoder_step(line, np.zeros((B, case.V), np.float32), states, a0)
    if case.family == 'uniform':
        assert np.array_equal(_bits(p1), _bits(np.full((B, case.V), np.float32(1) / np.float32(case.V), np.float32)))
        return
    g = groups_of(case.V, case.family[1], case.family[2])
    first = np.array([np.flatnonzero(g == g[v])[0] for v in range(case.V)])
    assert np.array_equal(_bits(p1), _bits(p1[:, first]))                 # identical E rows: identical probabilities
    assert len(np.unique(p1[0])) > 1
    p2, st2 = eng.decoder_step(line, p1, st1[:-1], st1[-1])
    assert np.array_equal(_bits(p2), _bits(p1))                           # the state is held: fast_sigmoid(30) == 1, fast_tanh(0) == 0
    for a, b in zip(st1[:-1], st2[:-1]):
        assert np.array_equal(_bits(a), _bits(b))


def _decode(eng, case, idx):
    """-> per line a list of results, each a dict of arrays cut to the result's length (what lies beyond is not defined)."""
    B, T = idx.shape
    MR = case.max_results
    eng.encode(idx)
    res = eng.decode_beam(want_align=True, **case.decoder_kwargs())
    S = res['idx'].shape[1]
    lo, w = eng.alignments_sparse(B * MR, S)
    out = []
    for j in range(B):
        rows = []
        for k in range(min(int(res['n_found'][j]), MR, 64)):
            r = j * MR + k
            n = int(res['len'][r])
            rows.append(dict(idx=res['idx'][r, :n].copy(), prob=res['prob'][r, :n].copy(), rej=res['rej'][r, :n].copy(),
                             score=res['score'][r].copy(), align=res['align'][r, :n].copy(), lo=lo[r, :n].copy(), w=w[r, :n].copy()))
        out.append(dict(n_found=int(res['n_found'][j]), n_steps=int(res['n_steps'][j]), results=rows,
                        empty=res['len'][j * MR + len(rows):(j + 1) * MR].copy()))
    return out


VARIANTS = [(c.name, a, False) for c in CASES for a in (0, 2)] + [(c.name, a, True) for c in CASES if c.lm for a in (0, 2)]


@pytest.mark.parametrize('name,arithmetic,lm', VARIANTS)
def test_the_search_on_a_tie_model_equals_the_oracle(name, arithmetic, lm):
    """The final list.  casv_decode_beam keeps the best f_cap = 64 finished hypotheses of a line, in order, and counts all of them
    (beam_step_kernel phase C: an insertion at `ppos < f_cap` shifts the tail down from slot f_cap - 1 and drops the worst entry,
    `ftot` counts every one; nothing is written beyond the list).  It returns at most max_results <= 64 of them and the stop test
    reads only the best entry and the count, so a line with more than 64 finished hypotheses loses nothing that can be returned:
    the cases h_finals_n64_lm (66), h_finals_n256 (249, 154 of them filed by one pop, the walk going on beyond the pop_cap = N + 64
    entries held in LDS) and h_finals_v1100_n256 (244) pin that -- n_found is the oracle's count, the 64 results returned are the
    oracle's first 64."""
    case = BY_NAME[name]
    m, idx, want = _expected(case, lm)
    B = len(case.lines)
    eng = _engine(case, arithmetic, lm)
    try:
        _preconditions(eng, case, idx)
        batch = _decode(eng, case, idx)
        most = eng.stat('beam_max_new_keys')
        capacity = eng.stat('beam_sort_capacity')
        alone = [_decode(eng, case, idx[j:j + 1])[0] for j in range(B)]
        backwards = _decode(eng, case, idx[::-1].copy())[::-1]
    finally:
        eng.close()
    _against_the_oracle(case, batch, want, m.mapping[0])
    _same_bits(batch, alone, 'each line alone')
    _same_bits(batch, backwards, 'lines reversed')
    assert most == max(tr['new_keys_max'] for _, _, _, tr in want), most
    if 'big_sort' in case.promises:
        assert (most > capacity) == case.promises['big_sort'], (most, capacity)
    if case.promises.get('over_f_cap'):
        assert max(d['n_found'] for d in batch) > 64 and max(len(d['results']) for d in batch) == case.max_results


def test_the_table_runs_both_sort_forms_and_overflows_the_final_list():
    assert {c.promises.get('big_sort') for c in CASES} >= {True, False}
    assert sum(bool(c.promises.get('over_f_cap')) for c in CASES) >= 2 and any(c.promises.get('many_finals') for c in CASES)
