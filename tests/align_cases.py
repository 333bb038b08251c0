"""The confusion network voted from candidate lines (include/cor_asv_ann_hip.h, casv_consensus_align and
casv_consensus_vote) restated on the host, the cases the device is held to, and a stub engine that answers from the restatement.

Everything here is exact: `where`, `ncol`, `src` and `best` are integers, and a mass is a float64 sum formed one IEEE addition at a
time in ascending candidate order from +0.0, so the device's results are compared bit for bit and no bound is needed.
tests/test_align_cases.py holds this file on the CPU, tests/test_gpu_confusion.py runs its cases on the device.
"""
import functools

import numpy as np

from tests import consensus_cases as cc

NONE = -2 ** 31                 # CASV_ALIGN_NONE
MAX_N, MAX_L = 256, 2048
WORD = 32                       # candidate symbols per direction word of consensus_align_kernel


# ------------------------------------------------------------------------------------------------------------------ the definition
def matrix(p, c):
    """D (len(p) + 1, len(c) + 1) int64: the unit-cost Levenshtein matrix of p[:i] against c[:j], row by row; the chain along a
    row, D[i][j-1] + 1, is a running minimum of (value - j) + j."""
    p, c = np.asarray(p, np.int64), np.asarray(c, np.int64)
    ramp = np.arange(len(c) + 1, dtype=np.int64)
    D = np.empty((len(p) + 1, len(c) + 1), np.int64)
    D[0] = ramp
    for i in range(1, len(p) + 1):
        row = np.empty(len(c) + 1, np.int64)
        row[0] = i
        np.minimum(D[i - 1, 1:] + 1, D[i - 1, :-1] + (c != p[i - 1]), out=row[1:])
        D[i] = np.minimum.accumulate(row - ramp) + ramp
    return D


def walk(p, c):
    """(where (len(c)) int64, the path's cost): the walk from (len(p), len(c)) to (0, 0) -- diagonal where it holds, else pivot
    against gap where that holds, else an insertion in slot i."""
    D = matrix(p, c)
    i, j = len(p), len(c)
    where = np.zeros(len(c), np.int64)
    cost = 0
    while i or j:
        if i and j and D[i, j] == D[i - 1, j - 1] + (p[i - 1] != c[j - 1]):
            where[j - 1] = i - 1
            cost += int(p[i - 1] != c[j - 1])
            i, j = i - 1, j - 1
        elif i and D[i, j] == D[i - 1, j] + 1:
            cost += 1
            i -= 1
        else:
            assert j and D[i, j] == D[i, j - 1] + 1
            where[j - 1] = -1 - i
            cost += 1
            j -= 1
    assert cost == D[-1, -1]
    return where, cost


_memo = {}


def _where(p, c):
    key = (p.tobytes(), c.tobytes())
    if key not in _memo:
        _memo[key] = walk(p, c)[0]
    return _memo[key]


def align_source(sym, length, pivot):
    """(where (N,L) int32, ncol, src (ncol,N) int32) of one source: sym (N,L), length (N) in -1 .. L, pivot in -1 .. N-1."""
    N, L = sym.shape
    where = np.full((N, L), NONE, np.int64)
    if pivot < 0:
        return where.astype(np.int32), 0, np.zeros((0, N), np.int32)
    assert length[pivot] >= 0
    lp = int(length[pivot])
    p = np.ascontiguousarray(sym[pivot, :lp], np.int32)
    ins = [0] * (lp + 1)
    for c in range(N):
        n = int(length[c])
        if n < 0:
            continue
        where[c, :n] = np.arange(n) if c == pivot else _where(p, np.ascontiguousarray(sym[c, :n], np.int32))
        count = [0] * (lp + 1)
        for v in where[c, :n]:
            if v < 0:
                count[-1 - v] += 1
        ins = [max(x, y) for x, y in zip(ins, count)]
    start, ncol = [], 0                 # the first column of slot g; the pivot's symbol g stands at start[g] + ins[g]
    for g in range(lp + 1):
        start.append(ncol)
        ncol += ins[g] + (1 if g < lp else 0)
    src = np.full((ncol, N), -1, np.int32)
    for c in range(N):
        n = int(length[c])
        if n < 0:
            src[:, c] = -2
            continue
        used = [0] * (lp + 1)
        for j in range(n):
            v = int(where[c, j])
            if v >= 0:
                col = start[v] + ins[v]
            else:
                col = start[-1 - v] + used[-1 - v]
                used[-1 - v] += 1
            assert src[col, c] == -1
            src[col, c] = j
    return where.astype(np.int32), ncol, src


def vote_source(sym, length, src, weight=None):
    """(mass (ncol,N) float64, best (ncol) int32): per column the classes -- the live candidates with a gap, those with equal
    symbols -- each at its lowest index with the members' weights added in ascending order as Python floats from +0.0; -1.0
    elsewhere; best = the first representative of the largest mass."""
    ncol, N = src.shape
    mass = np.full((ncol, N), -1.0, np.float64)
    best = np.full((ncol,), -1, np.int32)
    for col in range(ncol):
        rep, total = {}, {}
        for k in range(N):
            if length[k] < 0:
                continue
            key = ('gap',) if src[col, k] < 0 else (int(sym[k, src[col, k]]),)
            if key not in rep:
                rep[key], total[key] = k, 0.0
            total[key] = total[key] + (1.0 if weight is None else float(weight[k]))
        top = None
        for key, k in rep.items():      # (in order of the representatives' indices)
            mass[col, k] = total[key]
            if top is None or total[key] > mass[col, top]:
                top = k
        best[col] = top
    return mass, best


class Reference(object):
    """What a call pair returns: align(sym, length, pivot) -> (where (B,N,L), ncol (B)), then vote(C, weights) -> (src (B,C,N),
    mass (B,C,N), best (B,C)) on the inputs of the last align."""

    def align(self, sym, length, pivot):
        sym, length, pivot = np.asarray(sym, np.int32), np.asarray(length, np.int32), np.asarray(pivot, np.int32)
        B, N, L = sym.shape
        where, ncol, self.src = np.empty((B, N, L), np.int32), np.empty((B,), np.int32), []
        seen = {}           # (a source met again in the call: the same answer)
        for b in range(B):
            key = (sym[b].tobytes(), length[b].tobytes(), int(pivot[b]))
            if key not in seen:
                seen[key] = align_source(sym[b], length[b], int(pivot[b]))
            where[b], ncol[b], src = seen[key]
            self.src.append(src)
        self.sym, self.length = sym, length
        return where, ncol

    def vote(self, C, weights=None):
        B, N = self.length.shape
        assert C >= 1 and C >= max(len(s) for s in self.src)
        src, mass, best = np.full((B, C, N), -2, np.int32), np.full((B, C, N), -1.0, np.float64), np.full((B, C), -1, np.int32)
        seen = {}
        for b in range(B):
            w = None if weights is None else np.asarray(weights[b], np.float64)
            key = (self.sym[b].tobytes(), self.length[b].tobytes(), self.src[b].tobytes(), None if w is None else w.tobytes())
            if key not in seen:
                seen[key] = vote_source(self.sym[b], self.length[b], self.src[b], w)
            n = len(self.src[b])
            src[b, :n], (mass[b, :n], best[b, :n]) = self.src[b], seen[key]
        return src, mass, best


def reference(sym, length, pivot, weights=None, C=None):
    """(where, ncol, src, mass, best) of an align and one vote at C columns (None: the largest ncol, at least 1)."""
    ref = Reference()
    where, ncol = ref.align(sym, length, pivot)
    return (where, ncol) + ref.vote(max(1, int(ncol.max())) if C is None else C, weights)


def same(got, want):
    """Bit for bit, whatever the tuple holds: float64 masses through their int64 view, the integers as they are."""
    if len(got) != len(want):
        return False
    for g, w in zip(got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        if g.shape != w.shape or g.dtype != w.dtype:
            return False
        if g.dtype == np.float64:
            g, w = g.view(np.int64), w.view(np.int64)
        if not np.array_equal(g, w):
            return False
    return True


# ------------------------------------------------------------------------------------------------------------------ the cases
LENGTHS = [0, 1, 2, WORD - 1, WORD, WORD + 1, 63, 64, 65, 127, 128, 129, 200]     # the issue's, and one direction word -1 / exact / +1
SHAPE_N = [1, 2, 3, 64, 65, 256]
MANY_SOURCES = 66000        # beyond the 65535 sources a launch of any of the kernels takes side by side


def first_live(length):
    """Per source the first live candidate, -1 where there is none."""
    live = np.asarray(length) >= 0
    return np.where(live.any(axis=1), live.argmax(axis=1), -1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, sym (B,N,L), length (B,N), pivot (B), weights (B,N) float64 or None)]: what the issue lists, at the smallest sizes that
    reach every path of the kernels -- one strip of 64 pivot symbols, the strip boundary, several strips; one direction word of 32
    candidate symbols, its boundary, several words; the loops of the blocks over sources."""
    out = []
    # lengths against each other per alphabet: source b takes candidate b as its pivot, so every length meets every other as
    # pivot and as candidate; the pivot is the first, a middle and the last candidate on the way
    for name, alphabet in cc.ALPHABETS.items():
        rng = np.random.default_rng(100 + len(alphabet))
        base = cc._draw(rng, alphabet, 200)
        strings = [cc._mutate(rng, base[:n], alphabet, n // 8)[:n] if n else base[:0] for n in LENGTHS]
        strings = [np.concatenate([s, cc._draw(rng, alphabet, n - len(s))]) for s, n in zip(strings, LENGTHS)]
        sym, length = cc.pack(strings)
        B = len(LENGTHS)
        out.append(('lengths_' + name, np.repeat(sym[None], B, 0), np.repeat(length[None], B, 0), np.arange(B, dtype=np.int32), None))
    rng = np.random.default_rng(11)
    two = [0, -1]
    long = cc._draw(rng, two, MAX_L)
    near = np.concatenate([cc._mutate(rng, long[:1000], two, 90), long[1000:], cc._draw(rng, two, 200)])[:MAX_L - 1]
    packed = [cc.pack([long, near]), cc.pack([long, long[700:701]], L=MAX_L), cc.pack([long[900:901], long], L=MAX_L)]
    sym, length = cc._sources(*packed)
    assert length.tolist() == [[MAX_L, MAX_L - 1], [MAX_L, 1], [1, MAX_L]]
    out.append(('pairs_2048', sym, length, np.zeros(3, np.int32), None))
    # equal, first / last symbol changed, prefix and extension, reversed, around one and two strips: the base line as the pivot,
    # then its extension and its reverse
    four = [65, 67, 71, 84]
    for n in (64, 65, 130):
        base = cc._draw(rng, cc.ALPHABETS['many'], n)
        first, last = base.copy(), base.copy()
        first[0], last[-1] = first[0] ^ 1, last[-1] ^ 1
        strings = [base, base.copy(), first, last, base[:n - 1], base[:n // 2], np.concatenate([base, cc._draw(rng, four, 9)]), base[::-1].copy()]
        sym, length = cc.pack(strings)
        out.append(('structured_%d' % n, np.repeat(sym[None], 3, 0), np.repeat(length[None], 3, 0), np.array([0, 6, 7], np.int32), None))
    # the launch shape: N, and B with padding in front, in the middle, behind, sources of padding only and skipped sources
    pool = [cc._draw(rng, [0, 1], int(n)) for n in rng.integers(0, 7, 40)]
    for N in SHAPE_N:
        B = 17 if N == 256 else 1
        packed = [cc.pack([pool[int(k)] for k in rng.integers(0, len(pool), N)], L=6) for _ in range(B)]
        sym, length = cc._sources(*packed)
        out.append(('shape_N%d_B%d' % (N, B), sym, length, rng.integers(0, N, B).astype(np.int32), None))
    for B in (1, 3, 70):
        packed = []
        for b in range(B):
            strings = [cc._draw(rng, four, int(n)) for n in rng.integers(0, 12, 5)]
            for at in {0: (0,), 1: (2,), 2: (4,), 3: (0, 1, 3), 4: (0, 1, 2, 3, 4)}.get((b + B) % 7, ()):
                strings[at] = None
            packed.append(cc.pack(strings, L=11))
        sym, length = cc._sources(*packed)
        pivot = np.array([-1 if (length[b] < 0).all() or b % 9 == 5 else int(rng.choice(np.nonzero(length[b] >= 0)[0])) for b in range(B)], np.int32)
        out.append(('shape_N5_B%d_padding' % B, sym, length, pivot, None))
    few, few_len = cc.pack([[], [1], [0, 1], [1, 0], [1, 0, 1], [0, 0, 0], None])
    which = rng.integers(0, len(few), (MANY_SOURCES, 2))
    pivot = first_live(few_len[which])
    pivot[(few_len[which] >= 0).all(axis=1) & (np.arange(MANY_SOURCES) % 2 == 1)] = 1
    out.append(('sources_%d' % MANY_SOURCES, few[which], few_len[which], pivot, None))
    # weights over many magnitudes, zeros among them; lines that are noisy copies of one, so that the columns have real classes
    B, N = 6, 9
    packed = []
    for _ in range(B):
        base = cc._draw(rng, four, int(rng.integers(20, 41)))
        packed.append(cc.pack([cc._mutate(rng, base, four, int(e))[:40] for e in rng.integers(0, 9, N)], L=40))
    packed[2][1][[1, 5]] = -1
    sym, length = cc._sources(*packed)
    w = rng.random((B, N)) * 10.0 ** rng.integers(-12, 13, (B, N))
    w[rng.random((B, N)) < 0.2] = 0.0
    w[5] = np.ldexp(rng.random(N), rng.integers(-1000, 900, N))
    pivot = np.array([0, 8, 4, 3, 2, 1], np.int32)
    out.append(('weights', sym, length, pivot, w))
    out.append(('weights_none', sym, length, pivot, None))
    # exact ties: two classes of equal mass, the lower representative wins; all weights zero: every mass +0.0, the lowest wins
    x = cc._draw(rng, four, 30)
    y = x.copy()
    y[[3, 17, 29]] = 90
    packed = [cc.pack([x, y, y.copy(), x.copy()]), cc.pack([y, x, x.copy(), y.copy()]), cc.pack([None, y, x, None], L=30)]
    sym, length = cc._sources(*packed)
    out.append(('ties', sym, length, np.array([0, 3, 2], np.int32), None))
    out.append(('ties_weighted', sym, length, np.array([1, 0, 1], np.int32), np.array([[.5, .25, .25, 0.], [1., 3., 0., 2.], [9., 2., 2., 9.]])))
    out.append(('all_weights_zero', sym[:2], length[:2], np.array([2, 1], np.int32), np.zeros((2, 4))))
    # the order of the sum: one class of three, 1e16 + 1 + 1 = 1e16 but 1 + 1 + 1e16 = 1e16 + 2
    sym, length = cc._sources(cc.pack([x[:5]] * 3), cc.pack([x[:5]] * 3))
    out.append(('sum_order', sym, length, np.array([0, 2], np.int32), np.array([[1e16, 1., 1.], [1., 1., 1e16]])))
    return out


CASE_IDS = [c[0] for c in cases()]


def case(name):
    return cases()[CASE_IDS.index(name)][1:]


@functools.lru_cache(maxsize=None)
def expected(name):
    sym, length, pivot, w = case(name)
    return reference(sym, length, pivot, w)


# ------------------------------------------------------------------------------------------------------------------ a stub engine
class StubEngine(cc.StubEngine):
    """HipEngine.consensus, consensus_align and consensus_vote answered from the restatements; `calls` keeps every call's arguments."""

    def __init__(self):
        cc.StubEngine.__init__(self)
        self.ref = None

    def consensus_align(self, sym, length, pivot):
        sym, length, pivot = np.array(sym, np.int32), np.array(length, np.int32), np.array(pivot, np.int32)
        assert sym.ndim == 3 and length.shape == sym.shape[:2] and pivot.shape == sym.shape[:1]
        assert 1 <= sym.shape[1] <= MAX_N and sym.shape[2] <= MAX_L
        assert ((length >= -1) & (length <= sym.shape[2])).all()
        assert all(p == -1 or (0 <= p < sym.shape[1] and length[b, p] >= 0) for b, p in enumerate(pivot))
        self.calls.append(('align', sym, length, pivot))
        self.ref = Reference()
        return self.ref.align(sym, length, pivot)

    def consensus_vote(self, C, weights=None):
        assert self.ref is not None
        weights = None if weights is None else np.array(weights, np.float64)
        assert weights is None or (weights.shape == self.ref.length.shape and np.isfinite(weights).all() and (weights >= 0).all())
        self.calls.append(('vote', C, weights))
        return self.ref.vote(C, weights)
