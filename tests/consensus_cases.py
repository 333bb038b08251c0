"""The vote over candidate lines (include/cor_asv_ann_hip.h, casv_consensus) restated on the host, the cases
the device is held to, and a stub engine that answers from the restatement.

Everything here is exact: the distances are integers, and a risk is a float64 sum of products (mode 1: of a product with a quotient)
formed one IEEE operation at a time in ascending candidate order, so the device's results are compared bit for bit and no bound is
needed.  tests/test_consensus_cases.py holds this file on the CPU, tests/test_gpu_consensus.py runs its cases on the device.
"""
import functools

import numpy as np

I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31
ODD_SYMBOLS = [I32_MIN, -7, -1, 0, 1, 0x10FFFF, 0x110000, I32_MAX - 1, I32_MAX]      # negative, 0, the last code point, INT32_MAX
MAX_N, MAX_L = 256, 8192


# ------------------------------------------------------------------------------------------------------------------ the definition
def levenshtein(a, b):
    """Unit-cost edit distance of two sequences of ints: the row recurrence D[i][j] = min(D[i-1][j] + 1, D[i][j-1] + 1,
    D[i-1][j-1] + (a[i-1] != b[j-1])) with one numpy row per symbol of the shorter sequence (the distance is symmetric); the chain
    along the row, D[i][j-1] + 1, is a running minimum of (value - j) + j."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    if len(a) > len(b):
        a, b = b, a
    ramp = np.arange(len(b) + 1, dtype=np.int64)
    row = ramp.copy()
    for i in range(len(a)):
        new = np.empty_like(row)
        new[0] = i + 1
        np.minimum(row[1:] + 1, row[:-1] + (b != a[i]), out=new[1:])
        row = np.minimum.accumulate(new - ramp) + ramp
    return int(row[-1])


_memo = {}


def _distance(a, b):
    key = (a.tobytes(), b.tobytes())
    if key not in _memo:
        _memo[key] = _memo[key[::-1]] = levenshtein(a, b)
    return _memo[key]


def distance_matrix(sym, length):
    """D (N,N) int32 of one source: sym (N,L), length (N) in -1 .. L; -1 in the rows and columns of padding candidates."""
    N = len(length)
    live = [np.ascontiguousarray(sym[i, :length[i]], np.int32) if length[i] >= 0 else None for i in range(N)]
    D = np.full((N, N), -1, np.int32)
    for i in range(N):
        for j in range(i, N):
            if live[i] is not None and live[j] is not None:
                D[i, j] = D[j, i] = 0 if i == j else _distance(live[i], live[j])
    return D


def risk_and_pick(D, length, weight=None, mode=0):
    """(risk (N) float64, pick): risk[a] = the sum over the live candidates b in ascending order of w[b] * D[a][b] (mode 0) or
    w[b] * (D[a][b] / max(len[a], len[b], 1)) (mode 1) in Python floats, i.e. one IEEE float64 operation at a time from +0.0; +inf
    for a padding candidate.  pick = the first live candidate of the smallest risk, -1 without one."""
    N = len(length)
    risk = [float('inf')] * N
    for a in range(N):
        if length[a] < 0:
            continue
        total = 0.0
        for b in range(N):
            if length[b] < 0:
                continue
            d = float(int(D[a][b]))
            if mode == 1:
                d = d / float(max(int(length[a]), int(length[b]), 1))
            total = total + (1.0 if weight is None else float(weight[b])) * d
        risk[a] = total
    pick, best = -1, 0.0
    for a in range(N):
        if length[a] >= 0 and (pick < 0 or risk[a] < best):
            pick, best = a, risk[a]
    return np.array(risk, np.float64), pick


def reference(sym, length, weights=None, mode=0):
    """(risk (B,N) float64, pick (B) int32, dist (B,N,N) int32) of a whole call."""
    sym, length = np.asarray(sym, np.int32), np.asarray(length, np.int32)
    B, N = length.shape
    risk, pick, dist = np.empty((B, N), np.float64), np.empty((B,), np.int32), np.empty((B, N, N), np.int32)
    seen = {}           # (a source met again in the call, weights and all: the same answer)
    for b in range(B):
        key = (sym[b].tobytes(), length[b].tobytes(), None if weights is None else np.asarray(weights[b], np.float64).tobytes())
        if key not in seen:
            D = distance_matrix(sym[b], length[b])
            seen[key] = (D,) + risk_and_pick(D, length[b], None if weights is None else weights[b], mode)
        dist[b], risk[b], pick[b] = seen[key]
    return risk, pick, dist


def same(got, want):
    """Bit for bit: float64 risks through their int64 view, int32 picks and distances."""
    return (np.array_equal(np.ascontiguousarray(got[0], np.float64).view(np.int64), np.ascontiguousarray(want[0], np.float64).view(np.int64))
            and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]))


# ------------------------------------------------------------------------------------------------------------------ the cases
def pack(strings, L=None, fill=0):
    """One source from a list of int sequences (None: a padding candidate): (sym (N,L) int32, length (N) int32)."""
    L = max([len(s) for s in strings if s is not None] + [0]) if L is None else L
    sym = np.full((len(strings), L), fill, np.int32)
    length = np.full((len(strings),), -1, np.int32)
    for i, s in enumerate(strings):
        if s is not None:
            sym[i, :len(s)] = s
            length[i] = len(s)
    return sym, length


def _draw(rng, alphabet, n):
    return np.asarray(alphabet, np.int64)[rng.integers(0, len(alphabet), n)].astype(np.int32)


def _mutate(rng, s, alphabet, edits):
    s = list(s)
    for _ in range(edits):
        kind, at = rng.integers(0, 3), int(rng.integers(0, len(s) + 1))
        if kind == 0 and s:
            s[min(at, len(s) - 1)] = int(_draw(rng, alphabet, 1)[0])
        elif kind == 1 and s:
            del s[min(at, len(s) - 1)]
        else:
            s.insert(at, int(_draw(rng, alphabet, 1)[0]))
    return np.array(s, np.int32)


ALPHABETS = {'one': [5], 'two': [0, -1], 'many': ODD_SYMBOLS + list(range(32, 127))}
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 200]
SHAPE_N = [1, 2, 3, 64, 65, 256]
MANY_SOURCES = 66000        # beyond the 65535 sources a launch of either kernel takes side by side


def _sources(*packed):
    """Stack sources of one N into a call: (sym (B,N,L), length (B,N)), every source widened to the longest."""
    L = max(s.shape[1] for s, _ in packed)
    sym = np.zeros((len(packed), packed[0][0].shape[0], L), np.int32)
    for b, (s, _) in enumerate(packed):
        sym[b, :, :s.shape[1]] = s
    return sym, np.stack([l for _, l in packed])


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, sym (B,N,L), length (B,N), weights (B,N) float64 or None, mode)]: what the issue lists, at the smallest sizes that
    reach every path of the kernel -- one strip, the strip boundary at 64 rows, several strips, the longer string as rows or as
    columns, the loop of a block over sources (B beyond the launch's third grid dimension at N = 256)."""
    out = []
    # lengths against each other, per alphabet (mutated copies of one line, so that the distances are not just the length gaps)
    for name, alphabet in ALPHABETS.items():
        rng = np.random.default_rng(len(alphabet))
        base = _draw(rng, alphabet, 200)
        strings = [_mutate(rng, base[:n], alphabet, n // 8)[:n] if n else base[:0] for n in LENGTHS]
        strings = [np.concatenate([s, _draw(rng, alphabet, n - len(s))]) for s, n in zip(strings, LENGTHS)]
        sym, length = pack(strings)
        out.append(('lengths_' + name, sym[None], length[None], None, 0))
    rng = np.random.default_rng(7)
    four = [65, 67, 71, 84]
    a = _draw(rng, four, 700)
    sym, length = pack([a, np.concatenate([_mutate(rng, a[:600], four, 120), _draw(rng, four, 200)])[:650]])
    assert length.tolist() == [700, 650]
    out.append(('pair_700_650', sym[None], length[None], None, 0))
    long = _draw(rng, four, MAX_L)
    sym, length = pack([long, long[4000:4001]])
    out.append(('pair_8192_1', sym[None], length[None], None, 0))
    sym, length = pack([long, np.concatenate([_mutate(rng, long[:4000], four, 300), long[4000:], _draw(rng, four, 400)])[:MAX_L - 2]])
    assert length.tolist() == [MAX_L, MAX_L - 2]
    out.append(('pair_8192_8190', sym[None], length[None], None, 1))
    # equal, first / last symbol changed, prefix and extension, reversed: around one and two strips
    for n in (64, 65, 130):
        base = _draw(rng, ALPHABETS['many'], n)
        first, last = base.copy(), base.copy()
        first[0], last[-1] = first[0] ^ 1, last[-1] ^ 1
        strings = [base, base.copy(), first, last, base[:n - 1], base[:n // 2], np.concatenate([base, _draw(rng, four, 9)]), base[::-1].copy()]
        sym, length = pack(strings)
        out.append(('structured_%d' % n, sym[None], length[None], None, n % 2))
    # the launch shape: N, and B with padding at the start, in the middle, at the end, and a source of padding only
    pool = [_draw(rng, [0, 1], int(n)) for n in rng.integers(0, 7, 40)]
    for N in SHAPE_N:
        B = 17 if N == 256 else 1
        packed = [pack([pool[int(k)] for k in rng.integers(0, len(pool), N)], L=6) for _ in range(B)]
        sym, length = _sources(*packed)
        out.append(('shape_N%d_B%d' % (N, B), sym, length, None, 0))
    for B in (1, 3, 70):
        packed = []
        for b in range(B):
            strings = [_draw(rng, four, int(n)) for n in rng.integers(0, 12, 5)]
            for at in {0: (0,), 1: (2,), 2: (4,), 3: (0, 1, 3), 4: (0, 1, 2, 3, 4)}.get((b + B) % 7, ()):
                strings[at] = None
            packed.append(pack(strings, L=11))
        sym, length = _sources(*packed)
        out.append(('shape_N5_B%d_padding' % B, sym, length, None, B % 2))
    # more sources than a launch has blocks for: the blocks of both kernels loop over them
    few, few_len = pack([[], [1], [0, 1], [1, 0], [1, 0, 1], [0, 0, 0], None])
    which = rng.integers(0, len(few), (MANY_SOURCES, 2))
    out.append(('sources_%d' % MANY_SOURCES, few[which], few_len[which], None, 1))
    # weights over many magnitudes, zeros among them
    B, N = 6, 9
    packed = [pack([_draw(rng, four, int(n)) for n in rng.integers(0, 41, N)], L=40) for _ in range(B)]
    packed[2][1][[1, 5]] = -1
    sym, length = _sources(*packed)
    w = rng.random((B, N)) * 10.0 ** rng.integers(-12, 13, (B, N))
    w[rng.random((B, N)) < 0.2] = 0.0
    w[5] = np.ldexp(rng.random(N), rng.integers(-1000, 900, N))
    for mode in (0, 1):
        out.append(('weights_mode%d' % mode, sym, length, w, mode))
    # exact ties: duplicates have equal risks and the lower index wins; all weights zero: every risk +0.0, pick 0
    x, y, z = _draw(rng, four, 30), _draw(rng, four, 30), _draw(rng, four, 28)
    packed = [pack([x, y, y.copy(), x.copy(), z]), pack([z, x, y, x.copy(), y.copy()]), pack([None, y, x, y.copy(), None], L=30)]
    sym, length = _sources(*packed)
    for mode in (0, 1):
        out.append(('ties_mode%d' % mode, sym, length, None, mode))
    out.append(('all_weights_zero', sym[:2], length[:2], np.zeros((2, 5)), 0))
    return out


CASE_IDS = [c[0] for c in cases()]


@functools.lru_cache(maxsize=None)
def expected(name):
    _, sym, length, w, mode = cases()[CASE_IDS.index(name)]
    return reference(sym, length, w, mode)


def poisoned(sym, length, how, seed=0):
    """The call's symbols with every position at or beyond a candidate's length refilled: how = 'other' with the symbols the
    source's NEXT live candidate has there (so that the two would look equal further on), 'random' with random int32 values."""
    sym = np.array(sym, np.int32)
    B, N, L = sym.shape
    rng = np.random.default_rng(seed)
    noise = rng.integers(I32_MIN, I32_MAX, sym.shape, dtype=np.int64, endpoint=True).astype(np.int32)
    for b in range(B):
        for i in range(N):
            n = max(int(length[b, i]), 0)
            if how == 'random':
                sym[b, i, n:] = noise[b, i, n:]
            else:
                others = [j for j in list(range(i + 1, N)) + list(range(i)) if length[b, j] > n]
                sym[b, i, n:] = sym[b, others[0], n:] if others else noise[b, i, n:]
    return sym


# ------------------------------------------------------------------------------------------------------------------ a stub engine
class StubEngine(object):
    """HipEngine.consensus answered from the restatement; `calls` keeps every call's arguments."""

    def __init__(self):
        self.calls = []

    def consensus(self, sym, length, weights=None, mode=0, want_dist=False):
        sym, length = np.array(sym, np.int32), np.array(length, np.int32)
        assert sym.ndim == 3 and length.shape == sym.shape[:2]
        assert 1 <= sym.shape[1] <= MAX_N and sym.shape[2] <= MAX_L and mode in (0, 1)
        assert ((length >= -1) & (length <= sym.shape[2])).all()
        weights = None if weights is None else np.array(weights, np.float64)
        assert weights is None or (weights.shape == length.shape and np.isfinite(weights).all() and (weights >= 0).all())
        self.calls.append((sym, length, weights, mode, want_dist))
        risk, pick, dist = reference(sym, length, weights, mode)
        return risk, pick, (dist if want_dist else None)
