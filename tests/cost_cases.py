"""Weighted edit costs (include/cor_asv_ann_hip.h, casv_consensus_costed and casv_consensus_align_costed)
restated on the host, the wrong variants the cases must tell from the definition, the cases the device is held to, and a stub engine
that answers from the restatement.

The restatement is the header's text in plain numpy: the matrix row by row (the device sweeps anti-diagonals in strips), the walk by
the stated rule on the whole matrix (the device walks two bits per cell); risk, pick, the vote and the masses are those of
tests/consensus_cases.py and tests/align_cases.py.  Everything is exact -- the costs are integers -- so the device is compared bit
for bit.  tests/test_cost_cases.py holds this file on the CPU, tests/test_gpu_costed_consensus.py runs its cases on the device.
"""
import functools

import numpy as np

from tests import align_cases as ac
from tests import consensus_cases as cc

MAX_N, MAX_L = 256, 2048
UNIT = (1, 1, 1, 1)             # (gap, sub, near, unit): the plain calls

# What a wrong kernel could compute instead; every one must differ from the definition on a case of the list (test_cost_cases.py).
VARIANTS = ('near_as_sub',      # near charged as sub
            'keys_first',       # keys compared before symbols: equal symbols of equal keys cost near
            'unit_borders',     # row 0 and column 0 initialised with unit gaps
            'empty_no_gap',     # the shortcut for an empty string without gap
            'gap_bit_plus_1',   # the gap bit tested against up + 1
            'diag_bit_unit',    # the diagonal bit tested with the unit substitution cost
            'unit_ignored',     # mode 1 without unit
            'up_first')         # up preferred over the diagonal in the walk


# ------------------------------------------------------------------------------------------------------------------ the definition
def sub_cost(x, kx, y, ky, costs, variant=None):
    """c(x, y) for a symbol x with key kx against the symbols y with keys ky (arrays; ky None: no keys)."""
    _, sub, near, _ = costs
    if ky is None:
        return np.where(y == x, 0, sub)
    if variant == 'near_as_sub':
        near = sub
    if variant == 'keys_first':
        return np.where(ky == kx, near, np.where(y == x, 0, sub))
    return np.where(y == x, 0, np.where(ky == kx, near, sub))


def matrix(p, kp, c, kc, costs, variant=None):
    """D (len(p) + 1, len(c) + 1) int64 of p against c, row by row; the chain along a row, D[i][j-1] + gap, is a running minimum
    of (value - j * gap) + j * gap."""
    p, c = np.asarray(p, np.int64), np.asarray(c, np.int64)
    gap = costs[0]
    border = 1 if variant == 'unit_borders' else gap
    ramp = np.arange(len(c) + 1, dtype=np.int64) * gap
    D = np.empty((len(p) + 1, len(c) + 1), np.int64)
    D[0] = np.arange(len(c) + 1, dtype=np.int64) * border
    for i in range(1, len(p) + 1):
        row = np.empty(len(c) + 1, np.int64)
        row[0] = i * border
        np.minimum(D[i - 1, 1:] + gap, D[i - 1, :-1] + sub_cost(p[i - 1], None if kp is None else kp[i - 1], c, kc, costs, variant), out=row[1:])
        D[i] = np.minimum.accumulate(row - ramp) + ramp
    return D


def distance(a, ka, b, kb, costs, variant=None):
    if variant == 'empty_no_gap' and (len(a) == 0 or len(b) == 0):
        return max(len(a), len(b))
    return int(matrix(a, ka, b, kb, costs, variant)[-1, -1])


def walk(p, kp, c, kc, costs, variant=None):
    """where (len(c)) int64: from (len(p), len(c)), the diagonal where D[i][j] == D[i-1][j-1] + c(p[i-1], c[j-1]), else up where
    D[i][j] == D[i-1][j] + gap, else left -- an insertion in slot i."""
    D = matrix(p, kp, c, kc, costs, variant)
    gap = costs[0]
    i, j = len(p), len(c)
    where = np.zeros(len(c), np.int64)
    while j:
        diag = up = False
        if i:
            cost = int(sub_cost(p[i - 1], None if kp is None else kp[i - 1], c[j - 1:j], None if kc is None else kc[j - 1:j], costs, variant)[0])
            diag = D[i, j] == D[i - 1, j - 1] + (int(p[i - 1] != c[j - 1]) if variant == 'diag_bit_unit' else cost)
            up = D[i, j] == D[i - 1, j] + (1 if variant == 'gap_bit_plus_1' else gap)
            if variant == 'up_first' and up:
                diag = False
        if diag:
            where[j - 1] = i - 1
            i, j = i - 1, j - 1
        elif up:
            i -= 1
        else:
            where[j - 1] = -1 - i
            j -= 1
    return where


_memo = {}


def _pair(what, a, ka, b, kb, costs, variant):
    key = (what, a.tobytes(), None if ka is None else ka.tobytes(), b.tobytes(), None if kb is None else kb.tobytes(), costs, variant)
    if key not in _memo:
        _memo[key] = (distance if what == 'd' else walk)(a, ka, b, kb, costs, variant)
    return _memo[key]


def _live(sym, key, length, i):
    n = int(length[i])
    return np.ascontiguousarray(sym[i, :n], np.int32), None if key is None else np.ascontiguousarray(key[i, :n], np.int32)


def distance_matrix(sym, key, length, costs, variant=None):
    """D (N,N) int32 of one source; -1 in the rows and columns of padding candidates, 0 on the diagonal."""
    N = len(length)
    D = np.full((N, N), -1, np.int32)
    for i in range(N):
        for j in range(i, N):
            if length[i] >= 0 and length[j] >= 0:
                D[i, j] = D[j, i] = 0 if i == j else _pair('d', *_live(sym, key, length, i), *_live(sym, key, length, j), costs, variant)
    return D


def align_source(sym, key, length, pivot, costs, variant=None):
    """(where (N,L) int32, ncol, src (ncol,N) int32) of one source: tests/align_cases.py's with the costed walk."""
    N, L = sym.shape
    where = np.full((N, L), ac.NONE, np.int64)
    if pivot < 0:
        return where.astype(np.int32), 0, np.zeros((0, N), np.int32)
    lp = int(length[pivot])
    p, kp = _live(sym, key, length, pivot)
    for c in range(N):
        n = int(length[c])
        if n >= 0:
            where[c, :n] = np.arange(n) if c == pivot else _pair('w', p, kp, *_live(sym, key, length, c), costs, variant)
    live = [c for c in range(N) if length[c] >= 0]
    count = np.zeros((N, lp + 1), np.int64)                     # insertions of candidate c in slot g
    for c in live:
        v = where[c, :length[c]]
        np.add.at(count[c], -1 - v[v < 0], 1)
    ins = count.max(axis=0)
    start = np.concatenate([[0], np.cumsum(ins + 1)])[:lp + 1]          # the first column of slot g
    ncol = lp + int(ins.sum())
    src = np.full((ncol, N), -1, np.int32)
    src[:, [c for c in range(N) if length[c] < 0]] = -2
    for c in live:
        used = np.zeros(lp + 1, np.int64)
        for j in range(int(length[c])):
            v = int(where[c, j])
            if v >= 0:
                src[start[v] + ins[v], c] = j
            else:
                src[start[-1 - v] + used[-1 - v], c] = j
                used[-1 - v] += 1
    return where.astype(np.int32), ncol, src


def risk_and_pick(D, length, weight, mode, costs, variant=None):
    """tests/consensus_cases.py's risk over lengths scaled by unit: (double)D / (double)(unit * max(len, len, 1)), the product in
    integers -- the same IEEE operations in the same order."""
    unit = 1 if variant == 'unit_ignored' else costs[3]
    return cc.risk_and_pick(D, np.where(np.asarray(length) >= 0, np.maximum(np.asarray(length, np.int64), 1) * unit, -1), weight, mode)


class Reference(ac.Reference):
    """tests/align_cases.py's call pair with the costed alignment; the vote is its own."""

    def __init__(self, costs, variant=None):
        self.costs, self.variant = tuple(int(x) for x in costs), variant

    def align(self, sym, length, pivot, key=None):
        sym, length, pivot = np.asarray(sym, np.int32), np.asarray(length, np.int32), np.asarray(pivot, np.int32)
        key = None if key is None else np.asarray(key, np.int32)
        B, N, L = sym.shape
        where, ncol, self.src = np.empty((B, N, L), np.int32), np.empty((B,), np.int32), []
        seen = {}
        for b in range(B):
            live = np.arange(L)[None, :] < length[b][:, None]           # (what lies beyond a length is no part of the source)
            k = (np.where(live, sym[b], 0).tobytes(), None if key is None else np.where(live, key[b], 0).tobytes(), length[b].tobytes(), int(pivot[b]))
            if k not in seen:
                seen[k] = align_source(sym[b], None if key is None else key[b], length[b], int(pivot[b]), self.costs, self.variant)
            where[b], ncol[b], src = seen[k]
            self.src.append(src)
        self.sym, self.length = sym, length
        return where, ncol


def consensus(sym, key, length, weights, mode, costs, variant=None):
    """(risk (B,N) float64, pick (B) int32, dist (B,N,N) int32) of a casv_consensus_costed call."""
    sym, length = np.asarray(sym, np.int32), np.asarray(length, np.int32)
    key = None if key is None else np.asarray(key, np.int32)
    costs = tuple(int(x) for x in costs)
    B, N = length.shape
    L = sym.shape[2]
    risk, pick, dist = np.empty((B, N), np.float64), np.empty((B,), np.int32), np.empty((B, N, N), np.int32)
    seen = {}
    for b in range(B):
        live = np.arange(L)[None, :] < length[b][:, None]
        k = (np.where(live, sym[b], 0).tobytes(), None if key is None else np.where(live, key[b], 0).tobytes(), length[b].tobytes(),
             None if weights is None else np.asarray(weights[b], np.float64).tobytes())
        if k not in seen:
            D = distance_matrix(sym[b], None if key is None else key[b], length[b], costs, variant)
            seen[k] = (D,) + risk_and_pick(D, length[b], None if weights is None else weights[b], mode, costs, variant)
        dist[b], risk[b], pick[b] = seen[k]
    return risk, pick, dist


def reference(sym, key, length, pivot, weights, mode, costs, variant=None):
    """Every output of the two costed calls and one vote: (risk, pick, dist, where, ncol, src, mass, best)."""
    ref = Reference(costs, variant)
    where, ncol = ref.align(sym, length, pivot, key)
    return consensus(sym, key, length, weights, mode, costs, variant) + (where, ncol) + ref.vote(max(1, int(ncol.max())), weights)


same = ac.same      # bit for bit, whatever the tuple holds


# ------------------------------------------------------------------------------------------------------------------ the cases
LENGTHS = ac.LENGTHS                                    # 0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200
ALPHABETS = {'two': [0, 2], 'three': [0, 1, 2], 'four': [0, 1, 2, 3]}       # with keys sym mod 2: near pairs and ties everywhere
COST_SETS = [(1, 1, 1, 1), (1, 1, 0, 1), (2, 2, 1, 2), (2, 3, 1, 3), (1, 3, 0, 3), (1, 1, 1, 3)]
SHAPE_N = [1, 2, 3, 64, 65, 256]
MANY_SOURCES = 66000


def mod2(sym):
    return np.mod(sym, 2).astype(np.int32)


def _lengths(alphabet, seed):
    rng = np.random.default_rng(seed)
    base = cc._draw(rng, alphabet, 200)
    strings = [cc._mutate(rng, base[:n], alphabet, n // 8)[:n] if n else base[:0] for n in LENGTHS]
    return cc.pack([np.concatenate([s, cc._draw(rng, alphabet, n - len(s))]) for s, n in zip(strings, LENGTHS)])


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, sym (B,N,L), key (B,N,L) or None, length (B,N), pivot (B), weights (B,N) or None, mode, (gap, sub, near, unit))]:
    both costed calls run on every case.  Mode 1 wherever unit is not 1."""
    out = []

    def add(name, sym, key, length, pivot, w, costs, mode=None):
        out.append((name, sym, key, length, np.asarray(pivot, np.int32), w, (1 if costs[3] != 1 else 0) if mode is None else mode, costs))

    # every length against every other, as pivot and as candidate (source b takes candidate b as its pivot)
    B = len(LENGTHS)
    for name, alphabet in ALPHABETS.items():
        sym, length = _lengths(alphabet, 200 + len(alphabet))
        sym, length = np.repeat(sym[None], B, 0), np.repeat(length[None], B, 0)
        for costs in (COST_SETS if name == 'four' else [(1, 1, 0, 1), (2, 3, 1, 3)]):
            add('lengths_%s_%d_%d_%d_u%d' % ((name,) + costs), sym, mod2(sym), length, np.arange(B), None, costs)
    sym, length = _lengths(ALPHABETS['four'], 204)
    sym, length = np.repeat(sym[None], B, 0), np.repeat(length[None], B, 0)
    add('lengths_four_no_keys', sym, None, length, np.arange(B), None, (2, 3, 1, 3))
    rng = np.random.default_rng(23)
    add('lengths_four_keys_per_position', sym, rng.integers(0, 2, sym.shape).astype(np.int32), length, np.arange(B), None, (2, 2, 1, 2))
    # the longest pair, at the largest costs and at graded ones
    four = ALPHABETS['four']
    long = cc._draw(rng, four, MAX_L)
    other = np.concatenate([cc._mutate(rng, long[:1000], four, 90), long[1000:], cc._draw(rng, four, 200)])[:MAX_L]
    sym, length = cc.pack([long, other])
    assert length.tolist() == [MAX_L, MAX_L]
    add('pair_2048_max_costs', sym[None], mod2(sym)[None], length[None], [0], None, (255, 255, 255, 255))
    add('pair_2048_graded', sym[None], mod2(sym)[None], length[None], [1], None, (2, 2, 1, 2))
    # the distance kernel's choice of orientation
    a, b = cc._draw(rng, four, 3), cc._draw(rng, four, 65)
    sym, length = cc._sources(cc.pack([a, b]), cc.pack([b, a]))
    add('asymmetric_3_65', sym, mod2(sym), length, [0, 0], None, (2, 3, 1, 3))
    # the launch shape: N with padding candidates, sources of padding only, skipped sources, more sources than a launch takes
    pool = [cc._draw(rng, four, int(n)) for n in rng.integers(0, 7, 40)] + [None] * 6
    for N in SHAPE_N:
        B = 3 if N == 256 else 2
        packed = [cc.pack([pool[int(k)] for k in rng.integers(0, len(pool), N)], L=6) for _ in range(B)]
        sym, length = cc._sources(*packed)
        pivot = ac.first_live(length)
        pivot[1] = -1 if N == 3 else pivot[1]
        add('shape_N%d_B%d' % (N, B), sym, mod2(sym), length, pivot, None, (2, 2, 1, 2))
    few, few_len = cc.pack([[], [1], [0, 1], [2, 0], [1, 3, 1], [0, 0, 2], None])
    which = rng.integers(0, len(few), (MANY_SOURCES, 2))
    add('sources_%d' % MANY_SOURCES, few[which], mod2(few[which]), few_len[which], ac.first_live(few_len[which]), None, (1, 3, 0, 3))
    # odd values as symbols and as keys: the key of ODD_SYMBOLS[i] is ODD_SYMBOLS[i // 2]
    odd = np.array(cc.ODD_SYMBOLS, np.int64)
    strings = [cc._draw(rng, cc.ODD_SYMBOLS, int(n)) for n in (40, 37, 41, 0, 66)]
    sym, length = cc.pack(strings)
    key = odd[np.searchsorted(odd, sym) // 2].astype(np.int32)
    add('odd_symbols_and_keys', sym[None], key[None], length[None], [4], None, (2, 2, 1, 2))
    # weights over many magnitudes in both modes, noisy copies of one line
    B, N = 4, 9
    packed = []
    for _ in range(B):
        base = cc._draw(rng, four, int(rng.integers(20, 41)))
        packed.append(cc.pack([cc._mutate(rng, base, four, int(e))[:40] for e in rng.integers(0, 9, N)], L=40))
    packed[2][1][[1, 5]] = -1
    sym, length = cc._sources(*packed)
    w = rng.random((B, N)) * 10.0 ** rng.integers(-12, 13, (B, N))
    w[rng.random((B, N)) < 0.2] = 0.0
    for mode in (0, 1):
        add('weights_mode%d' % mode, sym, mod2(sym), length, [0, 8, 4, 3], w, (2, 3, 1, 3), mode)
    return out


CASE_IDS = [c[0] for c in cases()]


def case(name):
    return cases()[CASE_IDS.index(name)][1:]


@functools.lru_cache(maxsize=None)
def expected(name):
    return reference(*case(name))


def poisoned(sym, key, length, seed=0):
    """The call's symbols and keys with every position at or beyond a candidate's length refilled with what the source's next live
    candidate has there (so that the two would look equal further on), random int32 values where there is none."""
    return cc.poisoned(sym, length, 'other', seed), None if key is None else cc.poisoned(key, length, 'other', seed + 1)


# ------------------------------------------------------------------------------------------------------------------ a stub engine
class StubEngine(ac.StubEngine):
    """HipEngine.consensus / consensus_align: without costs tests/align_cases.py's stub, its calls recorded as they are today; with
    costs answered from the restatement here, recorded as ('costed', ...) and ('align_costed', ...)."""

    @staticmethod
    def _costs(costs):
        return tuple(int(x) for x in (costs.as_tuple() if hasattr(costs, 'as_tuple') else costs))

    def consensus(self, sym, length, weights=None, mode=0, want_dist=False, **costed):
        if not costed:
            return ac.StubEngine.consensus(self, sym, length, weights=weights, mode=mode, want_dist=want_dist)
        key, costs = costed.pop('key', None), self._costs(costed.pop('costs'))
        assert not costed and np.shape(sym)[2] <= MAX_L and (key is None or np.shape(key) == np.shape(sym))
        self.calls.append(('costed', np.array(sym, np.int32), None if key is None else np.array(key, np.int32), np.array(length, np.int32),
                           weights, mode, want_dist, costs))
        risk, pick, dist = consensus(sym, key, length, weights, mode, costs)
        return risk, pick, (dist if want_dist else None)

    def consensus_align(self, sym, length, pivot, **costed):
        if not costed:
            return ac.StubEngine.consensus_align(self, sym, length, pivot)
        key, costs = costed.pop('key', None), self._costs(costed.pop('costs'))
        assert not costed and np.shape(sym)[2] <= MAX_L and (key is None or np.shape(key) == np.shape(sym))
        self.calls.append(('align_costed', np.array(sym, np.int32), None if key is None else np.array(key, np.int32), np.array(length, np.int32),
                           np.array(pivot, np.int32), costs))
        self.ref = Reference(costs)
        return self.ref.align(sym, length, pivot, key)
