"""The device-packed result records at their edges -- test infrastructure, importable without a GPU (tests/test_record_cases.py
on the CPU, tests/test_gpu_records.py on the device).

pack_records_kernel (csrc/decode_kernels.hip) packs the best result of every line of the last decode call into a fixed-width
record; casv_records_reset / _append / _read / _device_ptr (csrc/engine.hip) and casv_comm_all_gather_records (csrc/comm.hip) sit
behind it.  Three things here:

the counting model   A random model does not reach the edges of the batched-greedy branch: its first end-of-line comes early or
                     never.  This one puts it where the input says.  Depth 1, width 32, V = 8, every tensor zero except: encoder
                     and decoder biases 30 on the forget gate (fl32(sigmoid(30)) == 1: c is a plain sum) and 1 on the output gate;
                     enc1_{fw,bw}_K[0, 2W:3W] = -KAPPA and the decoder's candidate-gate bias +KAPPA; E['\\n'] = (0.5, b, .., b),
                     E[a] = (0, -b, .., -b), E[x] = (1, 0, ..), E[y] = (40, 0, ..).  All units of a layer hold one value.  An input
                     character with first embedding entry e adds 0.5 * tanh(-KAPPA * e) to c: -d for an `x` (d = 0.5 tanh KAPPA =
                     0.0498), -d/2 for the '\\n', about -10 d for a `y`, nothing for padding, an unmapped character (E[0] = 0) or a
                     zero confidence.  The backward encoder's final c = -(n + 1/2) d for n `x` goes to the decoder, which adds d per
                     step (zero K and R: no feedback, no attention): c = (s - n + 1/2) d after step s.  All logits are h times the
                     row sum of E: `a` wins while c < 0, '\\n' from step n on.  The runner-up (a zero row of E) is 31 b |h| away,
                     0.56 b in the logit at |c| = d/2; from step n on it is `y`, (31 b - 39.5) |h| away.  b = 3 for the greedy cases (the
                     end-of-line's probability is 0.43 at step n: the score has something to sum), b = 8 for the beam (the search then returns a..a\\n of length n + 1; a line with twelve `y`
                     finishes nothing within 2T steps and falls back to its input -- with the rejection threshold 0: with the
                     default 0.3 a chain of rejection candidates can run along the source line to its '\n' and finish one, unless
                     an unmapped character or a zero confidence breaks the chain; the unfound cases therefore run with 0).

expected_records     the record of one decode call, restated in plain numpy and Python from the kernel's comments and
                     cor_asv_ann_amd/sharding.py -- not through strings, not through sharding.pack_records -- with one switch per
                     mistake a kernel of this kind can make (MUTATIONS; tests/test_record_cases.py shows that each changes a record
                     of the table).

the case table       CASES: the smallest shapes that reach every branch of the kernel.
"""
import math

import numpy as np

from oracle import ModelConfig, make_weights, make_vocabulary
from oracle.decode import OracleModel, decode_sequence_beam

WIDTH, V = 32, 8
KAPPA = 0.1
CFG = ModelConfig(depth=1, width=WIDTH, voc_size=V)
C_I, I_C = make_vocabulary(V)
EOS = C_I['\n']
CH_A, CH_X, CH_Y, CH_SPARE, CH_SPARE2, CH_SPARE3 = (I_C[k] for k in range(2, 8))      # ' ', '!', '"' and three zero rows of E
A_, X_, Y_, P_, Q_, R_ = range(2, 8)
UNMAPPED = '中'            # not in the vocabulary: index 0 through the reference's lookup (seq2seq.py:1078-1083)


# The greedy score has two computations: the record's (pack_records_kernel: -log of the probability as a double, summed in double)
# and the host path's (Sequence2Sequence._greedy_results: -np.log of the float32 probability in float32, summed in float64).
# Largest relative difference of the host path from the float64 restatement over the table's oracle probabilities, measured by
# tests/test_record_cases.py::test_the_greedy_score_of_the_host_path on 2026-10-18: 2.795e-08 = 0.47 * 2**-24.  Every term is
# non-negative, so the sum's relative error is at most the worst term's, half a float32 ulp of a correctly rounded log.  The bound
# for "host path against float64" is twice the measured value and never above 8 * 2**-24.
HOST_SCORE_MEASURED = 2.795e-08
HOST_SCORE_BOUND = min(2 * HOST_SCORE_MEASURED, 8 * 2.0 ** -24)


# ------------------------------------------------------------------------------------------------------------------ the model
def counting_weights(beta, dtype=np.float32):
    W = WIDTH
    w = {k: np.zeros_like(v) for k, v in make_weights(CFG).items()}
    for k in ('enc1_fw_b', 'enc1_bw_b', 'dec1_b'):
        w[k][W:2 * W] = 30.0
        w[k][3 * W:] = 1.0
    for k in ('enc1_fw_K', 'enc1_bw_K'):
        w[k][0, 2 * W:3 * W] = -KAPPA
    w['dec1_b'][2 * W:3 * W] = KAPPA
    E = w['E']
    E[EOS, 0], E[EOS, 1:] = 0.5, beta
    E[A_, 0], E[A_, 1:] = 0.0, -beta
    E[X_, 0] = 1.0
    E[Y_, 0] = 40.0
    return {k: v.astype(dtype) for k, v in w.items()}


# ------------------------------------------------------------------------------------------------------------------ inputs
def xs(n, head=''):
    """`head`, n copies of `x` and the end of the line."""
    return head + CH_X * n + '\n'


def sparse_lines(lines, conf=None):
    """Strings (and per-character confidences) -> (idx, val) (B, T, 1) as engine.encode takes them: -1 = padding, an unmapped
    character index 0 (seq2seq.py:1078-1083)."""
    B, T = len(lines), max(map(len, lines))
    idx = np.full((B, T, 1), -1, np.int32)
    val = np.zeros((B, T, 1), np.float32)
    for j, line in enumerate(lines):
        for t, ch in enumerate(line):
            idx[j, t, 0] = C_I.get(ch, 0)
            val[j, t, 0] = 1.0 if conf is None else conf[j][t]
    return idx, val


def slots(*lines):
    """Confusion-network lines given slot by slot: a line is a list of positions, a position a list of (index, value) or None
    (an empty slot) -> (idx, val) (B, T, A)."""
    B, T = len(lines), max(map(len, lines))
    A = max(len(pos) for line in lines for pos in line)
    idx = np.full((B, T, A), -1, np.int32)
    val = np.zeros((B, T, A), np.float32)
    for j, line in enumerate(lines):
        for t, pos in enumerate(line):
            for a, slot in enumerate(pos):
                if slot is not None:
                    idx[j, t, a], val[j, t, a] = slot
    return idx, val


def dense(idx, val):
    """(idx, val) -> the (B, T, V) float32 rows the reference vectorises the lines into."""
    B, T, A = idx.shape
    enc = np.zeros((B, T, V), np.float32)
    b, t, a = np.nonzero(idx >= 0)
    enc[b, t, idx[b, t, a]] = val[b, t, a]
    return enc


# ------------------------------------------------------------------------------------------------------------------ the record
MUTATIONS = ('last_eos', 'chunk_edge_early', 'chunk_edge_missed', 'pad_ignores_val', 'row_mul_ignored', 'fallback_skips_unmapped',
             'fallback_slot0', 'fallback_uncut', 'score_over_S')


def expected_records(idx, val, out, eos, S, mutate=None):
    """The records of one decode call.  idx / val (B, T[, A]): the inputs as passed to engine.encode; out: the arrays the decode
    call returned -- greedy: 'idx', 'prob' (B, S) of all S steps; beam: 'idx', 'prob' (B * max_results, S), 'len', 'score'
    (B * max_results,), the results of a line best first.  -> (B, 2S + 4) int32.

    Layout: characters in [0, S), probability bit patterns in [S, 2S), the length, the float64 score in two words (low, high), 1.
    Greedy: a line is padding if no slot has idx >= 0 and val != 0: all zero apart from the flag.  Otherwise the length runs up to
    and including the first end-of-line, or S; the score is the sum of -log(float64(p)) over the length, divided by it.
    Beam: result row j * max_results.  A line without a finished hypothesis (len == 0) is its input: the positions up to the last
    one that has any slot with idx >= 0, cut at S; per position the slot with the highest value, the lowest slot among equals, index
    0 where none; probabilities 1.0, score 0.
    mutate: one of MUTATIONS -- the same with one mistake."""
    assert mutate is None or mutate in MUTATIONS
    idx = np.asarray(idx, np.int32)
    idx = idx[:, :, None] if idx.ndim == 2 else idx
    B, T, A = idx.shape
    val = np.ones(idx.shape, np.float32) if val is None else np.asarray(val, np.float32).reshape(B, T, A)
    o_idx, o_prob = np.asarray(out['idx'], np.int32), np.asarray(out['prob'], np.float32)
    assert o_idx.shape[1] == S and o_prob.shape == o_idx.shape
    beam = out.get('len') is not None
    MR = o_idx.shape[0] // B
    assert o_idx.shape[0] == B * MR and (beam or MR == 1)
    rec = np.zeros((B, 2 * S + 4), np.int32)
    one = int(np.float32(1.0).view(np.int32))
    for j in range(B):
        row = j if mutate == 'row_mul_ignored' else j * MR
        chars, bits, n, score = [], [], 0, 0.0
        if beam and int(out['len'][row]) > 0:
            n = int(out['len'][row])
            score = float(out['score'][row])
            chars = [int(c) for c in o_idx[row, :n]]
            bits = [int(b) for b in o_prob[row, :n].view(np.int32)]
        elif beam:
            last = -1
            for t in range(T):
                if (idx[j, t] >= 0).any():
                    last = t
            for t in range(last + 1):
                if mutate == 'fallback_skips_unmapped' and not (idx[j, t] > 0).any():
                    continue
                c, best = 0, -1.0
                for a in range(A):
                    if idx[j, t, a] >= 0 and float(val[j, t, a]) > best:
                        c, best = int(idx[j, t, a]), float(val[j, t, a])
                    if mutate == 'fallback_slot0':
                        break
                chars.append(c)
            n = len(chars) if mutate == 'fallback_uncut' else min(len(chars), S)
            chars = chars[:S]
            bits = [one] * len(chars)
        else:
            live = (idx[j] >= 0) if mutate == 'pad_ignores_val' else ((idx[j] >= 0) & (val[j] != 0))
            if live.any():
                hits = [s for s in range(S) if o_idx[row, s] == eos]
                if mutate == 'chunk_edge_missed':
                    hits = [s for s in hits if s == 0 or s % 64]
                if mutate == 'chunk_edge_early':
                    hits = [s - 1 if s and s % 64 == 0 else s for s in hits]
                n = S if not hits else (hits[-1] if mutate == 'last_eos' else hits[0]) + 1
                total = math.fsum(-math.log(float(p)) for p in o_prob[row, :n])
                score = total / (S if mutate == 'score_over_S' else n)
                chars = [int(c) for c in o_idx[row, :n]]
                bits = [int(b) for b in o_prob[row, :n].view(np.int32)]
        rec[j, :len(chars)] = chars
        rec[j, S:S + len(bits)] = bits
        rec[j, 2 * S] = n
        rec[j, 2 * S + 1:2 * S + 3] = np.array([score], np.float64).view(np.int32)
        rec[j, 2 * S + 3] = 1
    return rec


def first_eos(o_idx, eos):
    """Per row the first step with `eos`, -1 where there is none."""
    hit = np.asarray(o_idx) == eos
    return np.where(hit.any(axis=1), hit.argmax(axis=1), -1)


def nonpad(idx, val):
    idx = np.asarray(idx)
    idx = idx[:, :, None] if idx.ndim == 2 else idx
    return ((idx >= 0) & (np.asarray(val).reshape(idx.shape) != 0)).any(axis=(1, 2))


# ------------------------------------------------------------------------------------------------------------------ cases
class Case(object):
    """One decode call (per entry of `steps`: None = the default 2T).  kind 'greedy' or 'beam'.
    counts (greedy): per line the planned first end-of-line step at unlimited S (a step >= S: none), None for a padding line.
    found (beam): per line whether the search finishes a hypothesis.
    lines / conf: the same input as strings (and confidences) for the host path, where it has that form."""

    def __init__(self, name, kind, idx, val, steps=(None,), counts=None, found=None, beta=3.0, max_results=1, rejection=0.3, lines=None,
                 conf=None):
        self.name, self.kind, self.idx, self.val, self.steps = name, kind, idx, val, tuple(steps)
        self.counts, self.found, self.beta, self.max_results, self.lines, self.conf = counts, found, beta, max_results, lines, conf
        self.rejection = rejection
        self.B, self.T, self.A = idx.shape

    def S(self, steps=None):
        return int(steps or 2 * self.T)

    def weights(self, dtype=np.float32):
        return counting_weights(self.beta, dtype)

    def model(self, dtype=np.float32):
        return OracleModel(CFG, self.weights(dtype), batch_size=4, rejection_threshold=self.rejection)

    def beam_kwargs(self):
        return dict(batch_size=4, max_results=self.max_results, rejection_threshold=self.rejection)

    def planned_eos(self, S):
        """Per line: the first end-of-line step, -1 for none within S steps, None for a padding line."""
        return [None if n is None else (n if n < S else -1) for n in self.counts]


def _strings(name, kind, lines, conf=None, **kw):
    idx, val = sparse_lines(lines, conf)
    return Case(name, kind, idx, val, lines=lines, conf=conf, **kw)


CHUNK_COUNTS = [0, 1, 2, 31, 62, 63, 64, 65, 100, 127, 128, 129]
_chunk_lines = [xs(n) for n in CHUNK_COUNTS] + ['', xs(5)]
_chunk_conf = [[1.0] * len(t) for t in _chunk_lines[:-1]] + [[0.0] * len(_chunk_lines[-1])]
_chunk_counts = CHUNK_COUNTS + [None, None]

_Y12 = CH_Y * 12
_unfound_lines = [xs(2, _Y12), xs(6), _Y12 + UNMAPPED + CH_X + '\n', xs(3, _Y12)]
_unfound_conf = [[1.0] * len(t) for t in _unfound_lines]
_unfound_conf[3][12] = _unfound_conf[3][14] = 0.0

_y = [(Y_, 1.0)]
_nl = [(EOS, 1.0)]
_pair = lambda n: [[(X_, 0.75), (P_, 0.25)]] * n

CASES = [
    # --- batched greedy: the first end-of-line either side of a 64-lane ballot chunk, a second chunk without a hit before the hit,
    #     an all-padding line (idx = -1) and a line with val = 0 everywhere
    _strings('greedy_chunks', 'greedy', _chunk_lines, _chunk_conf, counts=_chunk_counts),
    # --- end-of-line at S - 1; at step S, so none and length S; S a multiple of 64 and one past it
    _strings('greedy_cut', 'greedy', _chunk_lines, _chunk_conf, counts=_chunk_counts, steps=(64, 65, 128, 129)),
    # --- S < 64
    _strings('greedy_short', 'greedy', [xs(0), xs(1), xs(4)], counts=[0, 1, 4]),
    # --- A = 2 slots, 0.75 / 0.25 (an `x` at 0.75 counts three quarters: 8 of them 6 steps, 4 of them 3); a line whose only
    #     non-zero values sit in slot 1 (six `x` at 0.25: c = -1.5 d, end-of-line at step 1); padding decided over all T * A slots
    Case('greedy_confmat', 'greedy', *slots(_pair(8) + [_nl], _pair(4) + [_nl], [[(P_, 0.0), (X_, 0.25)]] * 6,
                                            [[(X_, 0.0), (P_, 0.0)]] * 3, [[None, (X_, 0.0)]] * 2), counts=[6, 3, 1, None, None]),
    # --- the beam: S = 82 > 64 in the copy loops; max_results = 4: the record is result 0 of the line
    _strings('beam_found', 'beam', [xs(3), xs(10), xs(40)], beta=8.0, found=[True] * 3),
    _strings('beam_mr4', 'beam', [xs(3), xs(10), xs(40)], beta=8.0, found=[True] * 3, max_results=4),
    # --- the fallback beside a found line in one batch: index 0 kept in place, a zero confidence still a character, truncation at
    #     S = 8 (below the line length)
    _strings('beam_unfound', 'beam', _unfound_lines, _unfound_conf, beta=8.0, rejection=0.0, found=[False, True, False, False],
             steps=(None, 8)),
    # --- the per-position choice, A = 3: distinct values, two equal values (first and later slots), a position with no slot and
    #     one with an empty slot 0 in the middle of a line, the highest value in the last slot
    Case('beam_unfound_confmat', 'beam', *slots(
        [_y] * 12 + [[(A_, 0.2), (X_, 0.5), (P_, 0.3)], [(P_, 0.3), (A_, 0.2), (X_, 0.5)], _nl],
        [_y] * 12 + [[(X_, 0.4), (P_, 0.4), (A_, 0.2)], [(A_, 0.2), (Q_, 0.4), (P_, 0.4)], _nl],
        [_y] * 12 + [[(X_, 1.0)], [], [None, (P_, 0.5), (A_, 0.25)], [(X_, 1.0)], _nl],
        [_y] * 12 + [[(A_, 0.1), (P_, 0.2), (X_, 0.7)], _nl]), beta=8.0, rejection=0.0, found=[False] * 4),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
VARIANTS = [(c.name, s) for c in CASES for s in c.steps]


# ------------------------------------------------------------------------------------------------------------------ the oracle
def oracle_greedy(case):
    """oracle.decode.decode_batch_greedy's loop on the case's model for its default 2T steps (a decode of fewer steps is a prefix)
    -> dict(idx (B, 2T) int32, prob (B, 2T) float32, gap: the smallest logit distance between the winner and the runner-up among
    the indices the greedy mode looks at (1..V-1), over all steps of all lines that are not padding)."""
    m = case.model()
    enc_in = dense(case.idx, case.val)
    enc = m.encode(enc_in)
    enc_out, states = enc[0], enc[1:]
    B, T = case.B, case.T
    p_in = np.zeros((B, V), np.float32)
    o_idx = np.zeros((B, 2 * T), np.int32)
    o_prob = np.zeros((B, 2 * T), np.float32)
    live = nonpad(case.idx, case.val)
    gap = np.inf
    for s in range(2 * T):
        scores, states = m.step(p_in, enc_out, states)
        pick = np.nanargmax(scores[:, 1:], axis=1) + 1
        o_idx[:, s] = pick
        o_prob[:, s] = scores[np.arange(B), pick]
        with np.errstate(divide='ignore'):
            ordered = np.sort(np.log(scores[:, 1:].astype(np.float64)), axis=1)
        gap = min(gap, float((ordered[:, -1] - ordered[:, -2])[live].min()))
        p_in = scores
    return dict(idx=o_idx, prob=o_prob, gap=gap)


def oracle_beam(case):
    """oracle.decode.decode_sequence_beam per line -> the arrays casv_decode_beam returns, for S = 2T steps: idx, prob
    (B * max_results, S), len, score (B * max_results,), n_found (B,); the strings of the results of every line."""
    m = case.model()
    enc_in = dense(case.idx, case.val)
    enc = m.encode(enc_in)
    B, MR, S = case.B, case.max_results, case.S()
    out = dict(idx=np.zeros((B * MR, S), np.int32), prob=np.zeros((B * MR, S), np.float32), len=np.zeros(B * MR, np.int32),
               score=np.zeros(B * MR, np.float64), n_found=np.zeros(B, np.int32), texts=[])
    for j in range(B):
        stats = {}
        res = list(decode_sequence_beam(m, source_seq=enc_in[j], encoder_outputs=[e[j:j + 1] for e in enc], stats=stats))
        out['n_found'][j] = stats['finals']
        out['texts'].append([r[0] for r in res])
        for k, (text, probs, score, _) in enumerate(res[:MR]):
            r = j * MR + k
            out['idx'][r, :len(text)] = [C_I[ch] for ch in text]
            out['prob'][r, :len(text)] = probs
            out['len'][r], out['score'][r] = len(text), score
    return out


_oracle = {}


def oracle_of(case):
    """The oracle's arrays of a case, computed once: oracle_greedy (every case: the gap) and, for the beam cases, oracle_beam."""
    if case.name not in _oracle:
        _oracle[case.name] = (oracle_greedy(case), oracle_beam(case) if case.kind == 'beam' else None)
    return _oracle[case.name]


def oracle_out(case, steps=None):
    """What the decode call of (case, steps) returns, from the oracle: the first S steps of the greedy matrices; the beam's arrays
    cut to S columns (the table's results that are found are shorter than its smallest S, the others have no columns)."""
    S = case.S(steps)
    g, b = oracle_of(case)
    if case.kind == 'greedy':
        return dict(idx=g['idx'][:, :S], prob=g['prob'][:, :S])
    assert int(b['len'].max()) <= S
    return dict(idx=b['idx'][:, :S], prob=b['prob'][:, :S], len=b['len'], score=b['score'])
