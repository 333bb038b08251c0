"""Cases, float64 reference and comparator for the train step's plain contractions in every launch form (csrc/train.hip, plain_gemm:
GemmArgs.ksplit = -1, kgroups = 2, accumulate, out_zeroed, row strides lda != K and ldc != N), host only.

tests/test_gpu_plain_sums.py runs every case through casv_debug_gemm_jobs_sum in every form the planner (csrc/gemm_plan.h) makes of
these fields and compares with the reference here; tests/test_plain_sum_cases.py pins the plans, shows that float32 arithmetic -- a
chain per K share, the shares added in any order -- passes the comparator and that every mutant of the reference (bias by every share,
a dropped share, the second wave group's tiles dropped, ...) does not.

The data conventions are those of tests/lstm_gemm_cases.py, whose builder, reference and comparator serve here: every pool row, pad
column and slot that nothing names is NaN, operands are scaled so that the product has unit deviation.  C0, what C holds before a
launch with `accumulate`, is drawn from N(0, 1).  The reference is C0 + A . Bt^T + bias in float64, the error is measured in units of
2^-24 (|C0| + sum|a||b| + |bias|), and the bounds are RMS_BOUND and MAX_BOUND of tests/test_gpu_gemm.py, which applies them to
split-K sums already: no constant is introduced here.

How a launch shares K out (gemm.hip, gemm_skinny.hip): the 128x128 tiles count K in tiles of 16, the 32- and 64-row tiles in stages
of 32; a launch of `shares` = grid_z shares gives each ceil(tiles / shares) tiles from the front, so the last share that holds any may
be short and the shares behind it hold none (they still run, and add zeros).  Share 0 alone adds the bias.  g128x2: the two wave
groups of a workgroup take the even and the odd tiles of the share and their accumulators are added before the epilogue.

THE CASES (M, N, K; each planned with tests/gemm_plan_driver.cpp at 256 CUs -- RUNS below holds forms, shares and clears of every run):
  edge         300, 198, 1024; lda = K + 32, ldc = 232.  Ragged rows and columns, padded rows.  ksplit = -1 gives 4 shares in every
               form: k32 (tile -1), g128 (tile 0), g128x2 (tile 0, kgroups 2), s128 (tile 0, split_bf16 1 and 2).
  uneven       300, 198, 1568.  98 tiles in 6 shares of 17, 17, 17, 17, 17, 13: odd counts for the two wave groups of g128x2; s128
               and g128 the same; k32: 49 stages in 6 shares of 9, 9, 9, 9, 9, 4.
  short_last   44, 96, 4128.  258 tiles in 16 shares, the last of 3 tiles (g128, g128x2: wave groups of 2 and 1 tile, s128); k32:
               129 stages in 16 shares of 9: the 15th holds 3, the 16th none.
  empty_share  44, 96, 10272.  642 tiles in 40 shares of 17: the 38th holds 13, two hold none; k32: 321 stages in 40 shares of 9:
               the 36th holds 6, four hold none.
  segments     300, 198, three gathered segments of widths 480 / 320 / 224 at koff 544 / 224 / 0: 4 shares of 256 k that straddle
               the borders at 480 and 800 (g128 at tile 0, k32).  No caller asks for this today; the planner admits it.
  natural_2wg  1100, 390, 1024 at tile -1 with kgroups 2: g128x2 in 4 shares under both arithmetics.
  natural_mid  2048, 512, 2048 at tile -1: arithmetic 0 -> g128 in 8 shares, arithmetic 2 -> s128 in 8 shares (what the train step
               takes at mid-size batches).
  cut32        8300, 1024, 64; lda 96, ldc 1056.  Arithmetic 0, ksplit -1: the partial round is cut, g128 (8192 rows) + k32 (108).
  cut64        12392, 1024, 64; 96, 1056: g128 (8192 rows) + k64 (4200 rows).
  cut256       8492, 2048, 64; 96, 2080.  Arithmetic 2, ksplit -1, kgroups 2: s256 (8192 rows) + k32 (300 rows: a launch that asks
               for split-K keeps the fp32-input small tiles); with accumulate the 256x256 tiles are out: s128 whole.

FORM x FIELD (every pair is either held by a run, or the planner never produces it: HELD below, checked by the CPU test):
               several shares   accumulate        out_zeroed        bias null    strides, ragged   ordered
  g128         held             held              held              held         held              held
  g128x2       held             held              held              held         held              held
  k32          held             held              held              held         held              held
  k64          never: 64-row tiles are chosen for launches without split-K only (gemm_choose_tiles: !splittable && ksplit == 1)
               --               held              held (no effect)  held         held              held
  s128         held             held              held              held         held              held
  s256         never: whole 256x256 tiles go as ONE share (plan_gemm_launches: ksplit == 1), and gemm_split256_job_ok refuses
               accumulate: such a job goes whole as s128 (cut256 with accumulate)
               --               never             held (no effect)  held         held (ldc, lda)   held
"""
import copy

import numpy as np

from tests import lstm_gemm_cases as lg
from tests.test_gpu_gemm import MAX_BOUND, RMS_BOUND

EPS = lg.EPS
NCU = 256
K_UNIT = {'g128': 16, 'g128x2': 16, 's128': 16, 's256': 16, 'k32': 32, 'k64': 32}       # what a form counts K in
FORMS = ('g128', 'g128x2', 'k32', 'k64', 's128', 's256')
FIELDS = ('shares', 'accumulate', 'out_zeroed', 'bias_null', 'strides', 'ordered')


class Run:
    """One launch of a case: the options, the launch fields, and what it must plan to at 256 CUs -- plan = [(form, shares)] in launch
    order, clears = clears of C in front of them."""

    def __init__(self, label, tile, arith, plan, clears=None, ksplit=-1, kgroups=0, accumulate=0, out_zeroed=0, bias=True, ordered=False):
        self.label, self.tile, self.arith, self.plan, self.bias, self.ordered = label, tile, arith, plan, bias, ordered
        self.fields = dict(ksplit=ksplit, kgroups=kgroups, accumulate=accumulate, out_zeroed=out_zeroed)
        shares = max(s for _, s in plan)
        self.clears = (1 if shares > 1 and not (accumulate or out_zeroed) else 0) if clears is None else clears

    @property
    def shares(self):
        return max(s for _, s in self.plan)

    def forms(self):
        return [f for f, _ in self.plan]


def _variants(label, tile, arith, plan, **kw):
    """a form with the plain settings, with accumulate, with out_zeroed and with bias null"""
    return [Run(label, tile, arith, plan, **kw), Run(label + '_acc', tile, arith, plan, accumulate=1, **kw),
            Run(label + '_zeroed', tile, arith, plan, out_zeroed=1, **kw), Run(label + '_nobias', tile, arith, plan, bias=False, **kw)]


def _pair(label, tile, arith, plan, **kw):
    return [Run(label, tile, arith, plan, **kw), Run(label + '_acc', tile, arith, plan, accumulate=1, **kw)]


def _every_form(make, k32, g128, more=()):
    """the four forms of a small shape in `k32` / `g128` shares (+ `more`)"""
    runs = make('k32', -1, 0, [('k32', k32)]) + make('g128', 0, 0, [('g128', g128)]) + make('g128x2', 0, 0, [('g128x2', g128)], kgroups=2)
    runs += make('s128_mode1', 0, 1, [('s128', g128)]) + make('s128_mode2', 0, 2, [('s128', g128)])
    return runs + list(more)


# the launches with ONE share, whose bits are compared (tests/test_gpu_plain_sums.py): every fp32-input form at ksplit 0 and under
# ordered sums, both split modes; g128x2 under ordered sums is what the deterministic train step runs
_EDGE_ONE = [r for tile, form in ((0, 'g128'), (1, 'k32'), (2, 'k64')) for r in _pair('one_' + form, tile, 0, [(form, 1)], ksplit=0)]
_EDGE_ONE += [Run('ordered_g128', 0, 0, [('g128', 1)], ordered=True), Run('ordered_k32', 1, 0, [('k32', 1)], ordered=True),
              Run('ordered_k32_natural', -1, 0, [('k32', 1)], ordered=True), Run('ordered_k64', 2, 0, [('k64', 1)], ordered=True),
              Run('ordered_g128x2', 0, 0, [('g128x2', 1)], kgroups=2, ordered=True),
              Run('ordered_g128x2_acc', 0, 0, [('g128x2', 1)], kgroups=2, ordered=True, accumulate=1),
              Run('one_s128_mode1', 0, 1, [('s128', 1)], ksplit=0), Run('one_s128_mode2', 0, 2, [('s128', 1)], ksplit=0),
              Run('one_s128_mode2_acc', 0, 2, [('s128', 1)], ksplit=0, accumulate=1),
              Run('ordered_s128_mode2', 0, 2, [('s128', 1)], ordered=True),
              Run('one_k64_zeroed', 2, 0, [('k64', 1)], ksplit=0, out_zeroed=1), Run('one_k64_nobias', 2, 0, [('k64', 1)], ksplit=0, bias=False)]

RUNS = {
    'edge': _every_form(_variants, 4, 4, _EDGE_ONE),
    'uneven': _every_form(_variants, 6, 6),
    'short_last': _every_form(_pair, 16, 16),
    'empty_share': _every_form(_pair, 40, 40),
    'segments': _pair('g128', 0, 0, [('g128', 4)]) + _pair('k32', -1, 0, [('k32', 4)]),
    'natural_2wg': _pair('g128x2_arith0', -1, 0, [('g128x2', 4)], kgroups=2) + _pair('g128x2_arith2', -1, 2, [('g128x2', 4)], kgroups=2),
    'natural_mid': _pair('g128', -1, 0, [('g128', 8)]) + _pair('s128', -1, 2, [('s128', 8)]),
    'cut32': _pair('cut', -1, 0, [('g128', 1), ('k32', 1)]) + _pair('one', -1, 0, [('g128', 1)], ksplit=0),
    'cut64': _pair('cut', -1, 0, [('g128', 1), ('k64', 1)]) + _pair('one', -1, 0, [('g128', 1)], ksplit=0),
    'cut256': [Run('cut', -1, 2, [('s256', 1), ('k32', 1)], kgroups=2), Run('cut_acc', -1, 2, [('s128', 1)], kgroups=2, accumulate=1),
               Run('cut_zeroed', -1, 2, [('s256', 1), ('k32', 1)], kgroups=2, out_zeroed=1),
               Run('cut_nobias', -1, 2, [('s256', 1), ('k32', 1)], kgroups=2, bias=False),
               Run('cut_ordered', -1, 2, [('s256', 1), ('k32', 1)], kgroups=2, ordered=True),
               Run('one', -1, 2, [('s256', 1), ('s128', 1)], ksplit=0), Run('one_fp32', -1, 0, [('g128', 1)], ksplit=0)],
}
# rows of the head launch of the cuts
CUT_ROWS = {'cut32': 8192, 'cut64': 8192, 'cut256': 8192}

# FORM x FIELD: 'held', or why the planner never produces the pair
_K64 = 'never: 64-row tiles are chosen for launches without split-K only (gemm_choose_tiles: !splittable && ksplit == 1)'
_S256 = 'never: whole 256x256 tiles go as one share (plan_gemm_launches asks for ksplit == 1)'
HELD = {(form, field): 'held' for form in FORMS for field in FIELDS}
HELD['k64', 'shares'] = _K64
HELD['s256', 'shares'] = _S256
HELD['s256', 'accumulate'] = 'never: gemm_split256_job_ok refuses accumulate, the job goes whole as s128 (cut256, cut_acc)'


def run_has(case, run, form, field):
    """whether `run` of `case` puts `field` on a launch of `form`"""
    if form not in run.forms():
        return False
    return {'shares': dict(run.plan)[form] > 1, 'accumulate': bool(run.fields['accumulate']), 'out_zeroed': bool(run.fields['out_zeroed']),
            'bias_null': not run.bias, 'strides': case.strided, 'ordered': run.ordered}[field]


class SumCase:
    """One shape: the job with its bias (lstm_gemm_cases.Job), C0, and the step it runs at"""

    def __init__(self, name, job, step, rng):
        self.name, self.job, self.step = name, job, step
        self.nobias = copy.copy(job)
        self.nobias.bias = None
        self.C0 = rng.standard_normal((job.M, job.N)).astype(np.float32)
        self.lg = lg.Case(name, 0, [job], (step,))
        self.strided = all(s.pool.shape[2] != s.width for s in job.segs) and job.out[1] != job.N        # lda != K, ldc != N
        self.runs = RUNS[name]
        self._base = self._operands = None

    def job_of(self, run):
        return self.job if run.bias else self.nobias

    def operands(self):
        """(A, Bt, order): A (M, Ktot) float64 as the kernels must read it, in Bt's columns; Bt float64 with the columns no segment
        names as zeros; order = Bt's columns in the order the kernels contract them (segment after segment).  Computed once."""
        if self._operands is not None:
            return self._operands
        job = self.job
        A = np.zeros((job.M, job.Ktot))
        order = []
        for sg in job.segs:
            A[:, sg.koff:sg.koff + sg.width] = sg.read(self.step, job.M)
            order.append(np.arange(sg.koff, sg.koff + sg.width))
        self._operands = A, np.where(job.covered(), job.Bt.astype(np.float64), 0.0), np.concatenate(order)
        for a in self._operands:
            a.setflags(write=False)
        return self._operands

    def base(self):
        """A . Bt^T and sum|a||b| in float64 (lstm_gemm_cases.reference of the job without bias): computed once, left unchanged"""
        if self._base is None:
            self._base = lg.reference(self.lg, self.nobias, self.step)
            self._base.z.setflags(write=False)
            self._base.mag.setflags(write=False)
        return self._base

    def reference(self, run):
        """C0 + A . Bt^T + bias in float64, with the magnitude the error is measured by"""
        base, r = self.base(), lg.Ref()
        r.live = base.live
        r.z, r.mag = base.z, base.mag
        if run.bias:
            r.z, r.mag = r.z + self.job.bias.astype(np.float64), r.mag + np.abs(self.job.bias.astype(np.float64))
        if run.fields['accumulate']:
            r.z, r.mag = r.z + self.C0.astype(np.float64), r.mag + np.abs(self.C0.astype(np.float64))
        return r

    def sums_of(self, run):
        """the `sums` entry of HipEngine.debug_gemm_jobs"""
        fields = dict(run.fields)
        if fields['accumulate']:
            fields['C0'] = self.C0
        return fields


def build_cases():
    """Every case, seeded by its place.  {name: SumCase}"""
    cases = []

    def add(name, M, N, widths, koffs=None, gather=None, big=False):
        rng = np.random.default_rng(2000 + len(cases))
        koffs = koffs or (0,)
        kw = dict(slots=1, out_slots=1) if big else {}      # (a chip-filling case: one slot, the pad columns and the guard row stay)
        step = 0 if big else 2
        job = lg.make_job(rng, M, N, widths, koffs, (step,), lstm=False, gather=gather or (False,) * len(widths), **kw)
        cases.append(SumCase(name, job, step, rng))
    add('edge', 300, 198, (1024,))
    add('uneven', 300, 198, (1568,))
    add('short_last', 44, 96, (4128,))
    add('empty_share', 44, 96, (10272,))
    add('segments', 300, 198, (480, 320, 224), (544, 224, 0), (True, True, True))
    add('natural_2wg', 1100, 390, (1024,))
    add('natural_mid', 2048, 512, (2048,))
    add('cut32', 8300, 1024, (64,), big=True)
    add('cut64', 12392, 1024, (64,), big=True)
    add('cut256', 8492, 2048, (64,), big=True)
    return {c.name: c for c in cases}


def plan_line(case, run):
    """the run as a line for tests/gemm_plan_driver.cpp"""
    job, f = case.job, run.fields
    csv = lambda fn: ','.join(str(fn(s)) for s in job.segs)      # noqa: E731
    mask = sum(1 << i for i, s in enumerate(job.segs) if s.rows is not None)
    return ('G %s_%s epi=0 ncu=%d tile=%d arith=%d ordered=%d ; M=%d N=%d segs=%s koffs=%s lds=%s Ktot=%d rows=%d outld=%d step=%d '
            'ksplit=%d kgroups=%d acc=%d zeroed=%d' % (case.name, run.label, NCU, run.tile, run.arith, int(run.ordered), job.M, job.N, csv(lambda s: s.width),
                                                        csv(lambda s: s.koff), csv(lambda s: s.pool.shape[2]), job.Ktot, mask, job.out[1], case.step,
                                                        f['ksplit'], f['kgroups'], f['accumulate'], f['out_zeroed']))


# ---- how a launch shares K out ----
def share_ranges(K, unit, shares):
    """[(k0, k1)] per share, in the kernels' K order: ceil(tiles / shares) tiles of `unit` each from the front; (k, k) = no tile"""
    tiles = K // unit
    per = (tiles + shares - 1) // shares
    return [(min(s * per, tiles) * unit, min((s + 1) * per, tiles) * unit) for s in range(shares)]


def passes(got, ref):
    rms, mx = lg.plain_errors(got, ref)
    return rms < RMS_BOUND and mx < MAX_BOUND


# ---- float32 as the kernels form the sum ----
def emulate(case, run, rng, form=None, shares=None):
    """(M, N) float32: per share ONE float32 chain over its 16-wide K tiles (each tile's product formed in float32), share 0 with the
    bias on top; then the shares added in a random order onto the cleared C, or onto C0"""
    A, Bt, order = case.operands()
    form = form or run.plan[0][0]
    shares = shares or run.shares
    A32, B32 = A[:, order].astype(np.float32), Bt[:, order].astype(np.float32)
    parts = []
    for s, (k0, k1) in enumerate(share_ranges(len(order), K_UNIT[form], shares)):
        acc = np.zeros((case.job.M, case.job.N), np.float32)
        for k in range(k0, k1, 16):
            acc = acc + A32[:, k:k + 16] @ B32[:, k:k + 16].T
        if s == 0 and run.bias:
            acc = acc + case.job.bias
        parts.append(acc)
    C = case.C0.copy() if run.fields['accumulate'] else np.zeros((case.job.M, case.job.N), np.float32)
    for s in rng.permutation(len(parts)):
        C = C + parts[s]
    return C


# ---- mutants of the reference ----
MUTANTS = ('bias_by_every_share', 'c0_ignored', 'c0_twice', 'last_share_dropped', 'first_tile_twice', 'second_group_dropped',
           'empty_share_contracts', 'tail_reads_a_with_k', 'tail_writes_c_with_n')


def mutant(case, run, name):
    """(M, N) float32 of what a launch with one fault would leave in rows < M, columns < N of the addressed slot; None: the fault
    does not apply to the run.  Faults of the sum act on the run's first launch form and its shares; the two faults of the cut on
    the tail launch behind it."""
    job, ref = case.job, case.reference(run)
    form, shares = run.plan[0]
    z = ref.z

    def product(k0, k1, sel=None):
        A, Bt, order = case.operands()
        cols = order[k0:k1] if sel is None else order[k0:k1][sel]
        return A[:, cols] @ Bt[:, cols].T
    ranges = share_ranges(sum(s.width for s in job.segs), K_UNIT[form], shares)
    full = [r for r in ranges if r[1] > r[0]]
    if name == 'bias_by_every_share':
        if not run.bias or shares < 2:
            return None
        z = z + (shares - 1) * job.bias.astype(np.float64)
    elif name in ('c0_ignored', 'c0_twice'):
        if not run.fields['accumulate']:
            return None
        z = z - case.C0 if name == 'c0_ignored' else z + case.C0
    elif name == 'last_share_dropped':
        if shares < 2:
            return None
        z = z - product(*full[-1])
    elif name == 'first_tile_twice':
        if shares < 2:
            return None
        z = z + product(ranges[1][0], ranges[1][0] + K_UNIT[form])
    elif name == 'second_group_dropped':
        if form != 'g128x2':
            return None
        for k0, k1 in full:                     # the odd tiles of every share
            odd = (np.arange(k1 - k0) // 16) % 2 == 1
            if odd.any():
                z = z - product(k0, k1, odd)
    elif name == 'empty_share_contracts':
        if len(full) == len(ranges):
            return None
        last = full[-1][1]
        z = z + (len(ranges) - len(full)) * product(last - K_UNIT[form], last)
    elif name in ('tail_reads_a_with_k', 'tail_writes_c_with_n'):
        if len(run.plan) < 2:
            return None
        head, M, N = CUT_ROWS[case.name], job.M, job.N
        out = z.astype(np.float32)
        if name == 'tail_reads_a_with_k':       # the tail's A starts head * K floats behind the base, not head * lda
            sg = job.segs[0]
            flat = sg.pool[sg.slot(case.step)].reshape(-1)
            lda = sg.pool.shape[2]
            at = head * sg.width + np.arange(M - head)[:, None] * lda + np.arange(sg.width)[None, :]
            with np.errstate(invalid='ignore'):
                wrong = flat[at].astype(np.float64) @ case.operands()[1].T
            wrong = wrong + (job.bias if run.bias else 0) + (case.C0[head:] if run.fields['accumulate'] else 0)
            out[head:] = wrong
            return out
        ldc = job.out[1]                        # the tail's C starts head * N floats behind the base, not head * ldc
        image = np.full((M + 1) * ldc, np.nan, np.float32)
        rows = image[:M * ldc].reshape(M, ldc)
        rows[:head, :N] = out[:head]
        if run.fields['accumulate']:
            rows[head:, :N] = case.C0[head:]
        at = head * N + np.arange(M - head)[:, None] * ldc + np.arange(N)[None, :]
        image[at] = out[head:]
        return rows[:, :N].copy()
    else:
        raise KeyError(name)
    return z.astype(np.float32)
