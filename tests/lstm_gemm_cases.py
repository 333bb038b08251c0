"""Cases, float64 reference and comparator for the operand machinery of the fused LSTM GEMM (csrc/gemm_args.h: K segments with
koff and ld, gathered rows, step addressing, the step-0 forms, the cell state, live rows, mixed batches), host only.

tests/test_gpu_lstm_gemm.py runs every case through casv_debug_gemm_jobs in every launch form that can take it and compares with
the reference here; tests/test_lstm_gemm_cases.py holds the reference to torch, shows that float32 arithmetic passes the comparator
and that every mutant of the reference (a dropped K tile, a wrong koff, an ungathered cell state ...) does not.

A case's pools are larger than its rows; what no index names is NaN: pool rows, the columns [width, ld) of every row, every slot
but the ones the case's steps select.  A kernel that reads a wrong row, column or slot shows as NaN or as a wrong number."""
import numpy as np

from tests.test_gpu_activations import ACT_BOUND
from tests.test_gpu_gemm import MAX_BOUND, RMS_BOUND

EPS = 2.0 ** -24
GATES = 4
BLOCK = 32              # units per 128-column block of the fused weight
FORM_BITS = {'g128': 0, 'g128x2': 1, 's128': 2, 'k32': 3, 'k64': 4, 's256': 5}        # GemmForm, csrc/gemm_plan.h


def form_mask(forms):
    return sum(1 << FORM_BITS[f] for f in forms)


def gate_columns(units):
    """(4, U): column of the fused weight that holds gate g of unit u -- the documented order [unit/32][gate i,f,c,o][unit%32]"""
    u = np.arange(units)
    return np.stack([(u // BLOCK) * (GATES * BLOCK) + g * BLOCK + u % BLOCK for g in range(GATES)])


class Part:
    """An input whose rows move with the step: K segment, cell state or zinit (casv_debug_rows)"""

    def __init__(self, pool, width, koff=0, rows=None, first=None, step_mul=1, step_add=0, skip_first=False):
        self.pool, self.width, self.koff, self.rows, self.first = pool, width, koff, rows, first
        self.step_mul, self.step_add, self.skip_first = step_mul, step_add, skip_first

    def slot(self, step):
        return step * self.step_mul + self.step_add

    def read(self, step, M, mutant=None):
        """(M, width) float64 as the kernels must read it at `step`; None: counts as zeros"""
        if step == 0 and self.first is not None:
            return self.first[:, :self.width].astype(np.float64)
        if step == 0 and self.skip_first and mutant != 'not_skipped':
            return None
        rows = np.arange(M) if self.rows is None or mutant == 'ungathered' else self.rows
        if mutant == 'swap_rows':
            rows = rows.copy()
            a, b = self.swap_pair
            rows[a], rows[b] = rows[b], rows[a]
        slot = self.slot(step)
        if mutant == 'slot_off':
            slot = slot + 1 if slot + 1 < self.pool.shape[0] else slot - 1
        return self.pool[slot, rows, :self.width].astype(np.float64)


class Job:
    def __init__(self, **kw):
        self.zinit = self.gates_out = self.out2 = self.c_in = self.c_out = self.nact = self.bias = None
        self.nact_group, self.b_static, self.epi_plain = 0, False, False
        self.__dict__.update(kw)

    def covered(self):
        """(Ktot,): the columns of Bt that a segment names"""
        k = np.zeros(self.Ktot, bool)
        for sg in self.segs:
            k[sg.koff:sg.koff + sg.width] = True
        return k

    def live(self):
        if self.nact is None:
            return np.ones(self.M, bool)
        m = np.arange(self.M)
        return m % self.nact_group < np.asarray(self.nact)[m // self.nact_group]


class Case:
    def __init__(self, name, epi, jobs, steps, forms=None):
        self.name, self.epi, self.jobs, self.steps, self.forms = name, epi, jobs, steps, forms or ALL_FORMS

    def lstm(self, job):
        return self.epi == 1 and not job.epi_plain


# ---- the builder ----
def _index(rng, M, pool_rows, live):
    """A permutation-like index into the pool that repeats some rows; dead rows name one pool row that no live row names"""
    perm = rng.permutation(pool_rows)
    rows, nan_row = perm[:M].copy(), perm[M]
    rep = rng.choice(M, max(2, M // 8), replace=False)
    rows[rep] = rows[rng.choice(M, len(rep))]
    rows[~live] = nan_row
    return rows.astype(np.int32)


def _part(rng, M, width, ld, steps, slots, live, gather, koff=0, mul=1, add=0, skip_first=False, first=False, draw=None, extra=41):
    draw = draw or (lambda shape: rng.standard_normal(shape))
    pool_rows = M + extra
    pool = np.full((slots, pool_rows, ld), np.nan, np.float32)
    rows = _index(rng, M, pool_rows, live) if gather else None
    named = np.unique(rows[live]) if gather else np.flatnonzero(live)
    for step in steps:
        s = step * mul + add
        if 0 <= s < slots:
            pool[s, named, :width] = draw((len(named), width))
    part = Part(pool, width, koff, rows, None, mul, add, skip_first)
    if first:
        part.first = np.full((M, ld), np.nan, np.float32)
        part.first[live, :width] = draw((int(live.sum()), width))
    if gather:          # two live rows that name different pool rows (the `swap_rows` mutant)
        lv = np.flatnonzero(live)
        part.swap_pair = (lv[0], next(m for m in lv[1:] if rows[m] != rows[lv[0]]))
    return part


def make_job(rng, M, N, widths, koffs, steps, *, lstm=True, gather=(True, True, False), bias=True, slots=3, seg_step=(1, 0),
             out_step=(1, 0), c_out_step=(1, 1), skip=(), first=(), c_skip=False, c_first=False, c_gather=True, nact=None, nact_group=0,
             side=False, b_static=False, epi_plain=False, pad=32, out_slots=None, Ktot=None):
    """One job.  Operands are scaled so that the pre-activations have standard deviation ~ 1 (a saturated cell would hide errors in
    z), c_prev is drawn from +-2.  steps: the steps the job will be run at (their slots are filled, every other slot is NaN)."""
    job = Job(M=M, N=N, Ktot=int(Ktot or sum(widths)), nact=None if nact is None else np.asarray(nact, np.int32), nact_group=nact_group,
              b_static=b_static, epi_plain=epi_plain)
    live = job.live()
    mul, add = seg_step
    out_slots = out_slots or slots + 1
    job.segs = [_part(rng, M, w, w + pad, steps, slots, live, gather[i], koffs[i], mul, add, i in skip, i in first)
                for i, w in enumerate(widths)]
    scale = 1.0 / np.sqrt(sum(widths))
    if lstm:
        U = N // GATES
        job.W = (rng.standard_normal((GATES, U, job.Ktot)) * scale).astype(np.float32)       # gate-major: what torch's LSTMCell takes
        job.b = (rng.standard_normal((GATES, U)) * 0.25).astype(np.float32)
        cols = gate_columns(U)
        job.Bt = np.empty((N, job.Ktot), np.float32)
        job.Bt[cols] = job.W
        if bias:
            job.bias = np.empty(N, np.float32)
            job.bias[cols] = job.b
        job.c_in = _part(rng, M, U, U + pad, steps, slots, live, c_gather, 0, mul, add, c_skip, c_first, draw=lambda shape: rng.uniform(-2, 2, shape))
        job.out = (out_slots, U + pad, out_step[0], out_step[1])
        job.c_out = (out_slots, U + 4, c_out_step[0], c_out_step[1])
        if side:
            zin = np.full((slots, M, N + pad), np.nan, np.float32)
            for step in steps:
                zin[step * mul + add, :, :N] = rng.standard_normal((M, N)) * 0.25
            job.zinit = Part(zin, N, 0, None, None, mul, add, False)
            job.gates_out = (out_slots, N + pad, out_step[0], out_step[1])
            job.out2 = (out_slots, U + 8, out_step[0], out_step[1])
    else:
        job.Bt = (rng.standard_normal((N, job.Ktot)) * scale).astype(np.float32)
        if bias:
            job.bias = (rng.standard_normal(N) * 0.25).astype(np.float32)
        job.out = (out_slots, (N + 3) // 4 * 4 + pad, out_step[0], out_step[1])
    job.Bt[:, ~job.covered()] = np.nan          # (columns of K that no segment names)
    return job


def _small(rng, M=300, steps=(2,), **kw):
    """M = 300: two full 128-row tiles and 44 ragged rows; N = 256: 64 units, so bn = 1 exists.  Segments x | h | ctx of widths
    32 / 64 / 32 with ld = width + 32; koff falls while the segments rise, so the K order differs from the order in memory."""
    return make_job(rng, M, 256, (32, 64, 32), (96, 32, 0), steps, **kw)


def _plain_rider(rng, M=200, steps=(2,), **kw):
    """the attention query's place in layer 1's launch: a plain-epilogue job of another N (96: ragged columns) and M; its segment
    lies inside a wider K (koff 16 of 96: columns of Bt that no segment names are NaN)"""
    return make_job(rng, M, 96, (64,), (16,), steps, Ktot=96, lstm=False, gather=(True,), epi_plain=True, **kw)


def _big(rng, M, steps=(0, 3), **kw):
    """One chip-filling shape for the 256x256 tiles: N = 2048, three segments, Ktot = 160 (short, so that the float64 product stays
    under a second on the host).  Gathered x and h, step 3, and (unless the caller says otherwise) the zero state of step 0 in one job."""
    for key, value in dict(slots=4, skip=(1,), c_skip=True, out_step=(0, 1), c_out_step=(0, 0), out_slots=2).items():
        kw.setdefault(key, value)
    return make_job(rng, M, 2048, (64, 64, 32), (96, 32, 0), steps, **kw)


SPLIT_FORMS = ('split1', 'split2_image', 'split2_staging')
ALL_FORMS = ('tile0', 'tile1', 'tile2') + SPLIT_FORMS


def build_cases():
    """Every case, seeded by its place.  {name: Case}"""
    cases = []

    def add(name, epi, jobs, steps, **kw):
        cases.append(Case(name, epi, jobs, steps, **kw))
    rng = lambda: np.random.default_rng(1000 + len(cases))      # noqa: E731
    # (a) segments and gather
    add('a_bias', 1, [_small(rng())], (2,))
    add('a_nobias', 1, [_small(rng(), bias=False)], (2,))
    # (b) step addressing: step 3, slot = step + 1 and 5 - step; c_out in slot step + 1 of a pool of its own; valid at step 0 too,
    # because a step that arrives through the device word leaves 0 in the arguments' immediate step
    add('b_step_plus', 1, [_small(rng(), steps=(3,), slots=6, seg_step=(1, 1), out_step=(1, 2), c_out_step=(1, 1))], (3,))
    add('b_step_minus', 1, [_small(rng(), steps=(3,), slots=6, seg_step=(-1, 5), out_step=(-1, 4), c_out_step=(1, 1))], (3,))
    # (c) step 0: the zero state; the initial state that comes ungathered from another base.  Step 1 reads the gathered pool.
    add('c_skip_first', 1, [_small(rng(), steps=(0, 1), skip=(1,), c_skip=True)], (0, 1))
    add('c_first_base', 1, [_small(rng(), steps=(0, 1), first=(1,), c_first=True)], (0, 1))
    # (d) mixed batches
    add('d_two_jobs', 1, [_small(rng()), _small(rng(), M=130)], (2,))
    add('d_plain_rider', 1, [_small(rng()), _plain_rider(rng())], (2,))
    add('d_four_jobs', 1, [_small(rng()), _small(rng(), M=130, bias=False), _plain_rider(rng()), _small(rng(), M=44)], (2,))
    # (e) live rows.  48-row lines, M = 384: line 2 = rows 96..143 straddles the 128-row boundary at offset 32; with 32 live rows
    # row 128 is dead and no tile shape has a live row in rows 128..255, with 33 it is live.
    for name, n2 in (('e_straddle_dead', 32), ('e_straddle_live', 33)):
        add(name, 1, [_small(rng(), M=384, nact=[48, 17, n2, 0, 0, 0, 20, 48], nact_group=48)], (2,))
    add('e_finished_lines', 1, [_small(rng(), M=1024, nact=[200, 0, 1, 0], nact_group=256)], (2,))
    # (f) the train step's side outputs, on the fp32-input forms
    add('f_side_outputs', 1, [_small(rng(), side=True)], (2,), forms=('tile0', 'tile1', 'tile2'))
    # a plain launch with segments, gather and ragged columns (every form has a plain epilogue of its own)
    add('p_plain_launch', 0, [make_job(rng(), 300, 200, (32, 64, 32), (96, 32, 0), (2,), lstm=False)], (2,))
    # the 256x256 tiles.  8448 rows: whole rounds as 256x256 tiles, the partial round as 128x128 split tiles; 8492: a ragged last
    # block too; 8192 rows of 8-row lines: live rows in 256x256 tiles; 8448 rows of 8-row lines: the cut must shift nact.
    add('s_8448', 1, [_big(rng(), 8448)], (0, 3), forms=SPLIT_FORMS)
    add('s_8492', 1, [_big(rng(), 8492)], (0, 3), forms=SPLIT_FORMS)
    for M in (8192, 8448):
        r = rng()
        nact = r.integers(0, 9, M // 8)
        nact[512 // 8:768 // 8] = 0             # one whole 256-row block finished
        nact[0] = 8
        if M > 8192:                            # the first 128 rows behind the cut finished, the rest of the tail live
            nact[8192 // 8:8320 // 8] = 0
            nact[8320 // 8:] = r.integers(1, 9, (M - 8320) // 8)
        add('s_%d_lines_of_8' % M, 1, [_big(r, M, nact=nact, nact_group=8)], (0, 3), forms=SPLIT_FORMS)
    # (c) in 256x256 tiles: the initial state of h and of the cell, ungathered from another base at step 0, gathered at step 3
    add('s_first_base', 1, [_big(rng(), 8448, skip=(), c_skip=False, first=(1,), c_first=True)], (0, 3), forms=SPLIT_FORMS)
    # (b) in 256x256 tiles: inputs in slot 5 - step, h in slot 3 - step, c_out in slot step + 1 (by immediate and by device word);
    # with it a plain-epilogue job of another N that fills the chip as 256x256 tiles too: a batch of two in that form
    add('s_step', 1, [_big(rng(), 8448, steps=(3,), slots=6, seg_step=(-1, 5), out_step=(-1, 3), c_out_step=(1, 1), out_slots=5, skip=(), c_skip=False),
                      make_job(rng(), 8192, 1024, (64,), (16,), (3,), Ktot=96, lstm=False, gather=(True,), epi_plain=True, slots=6,
                               seg_step=(1, 1), out_step=(0, 1), out_slots=2)], (3,), forms=SPLIT_FORMS)
    return {c.name: c for c in cases}


# what each option setting must become at 256 CUs (tests/test_lstm_gemm_cases.py plans every case; the GPU test reads the statistic)
OPTIONS = {'tile0': dict(tile=0, split_bf16=0), 'tile1': dict(tile=1, split_bf16=0), 'tile2': dict(tile=2, split_bf16=0),
           'split1': dict(tile=-1, split_bf16=1), 'split2_image': dict(tile=-1, split_bf16=2), 'split2_staging': dict(tile=-1, split_bf16=2)}
FP32_FORMS = ('tile0', 'tile1', 'tile2')


def intended_forms(case, form):
    if form in ('tile0', 'tile1', 'tile2', 'split1'):
        return [{'tile0': 'g128', 'tile1': 'k32', 'tile2': 'k64', 'split1': 's128'}[form]]
    M = case.jobs[0].M
    if case.jobs[0].N < 2048:           # too few 256x256 tiles to fill the chip: mode 2 runs as mode 1
        return ['s128']
    return ['s256'] if M == 8192 else ['s256', 's128']          # whole rounds; the partial round / ragged block behind the cut


def plan_line(case, form, step=None, name=None, head=''):
    """The case as a line for tests/gemm_plan_driver.cpp, under the options of `form` (b_static as the form wants it)"""
    opt = OPTIONS[form]
    jobs = []
    for job in case.jobs:
        lstm = case.lstm(job)
        mask = lambda pred: sum(1 << i for i, s in enumerate(job.segs) if pred(s))     # noqa: E731
        csv = lambda f: ','.join(str(f(s)) for s in job.segs)      # noqa: E731
        keys = ['M=%d N=%d segs=%s koffs=%s lds=%s Ktot=%d' % (job.M, job.N, csv(lambda s: s.width), csv(lambda s: s.koff), csv(lambda s: s.pool.shape[2]), job.Ktot),
                'rows=%d first=%d skip=%d' % (mask(lambda s: s.rows is not None), mask(lambda s: s.first is not None), mask(lambda s: s.skip_first)),
                'step=%d' % (case.steps[-1] if step is None else step)]
        if lstm and job.c_in.rows is not None:
            keys.append('crows=1')
        if job.epi_plain:
            keys.append('epiplain=1')
        if job.nact is not None:
            keys.append('nact=%d' % job.nact_group)
        if job.zinit is not None:
            keys.append('zinit=1 gates=1 out2=1')
        if form == 'split2_image' or job.b_static:
            keys.append('bstatic=1')
        jobs.append(' '.join(keys))
    head = ('epi=%d tile=%d arith=%d %s' % (case.epi, opt['tile'], max(opt['split_bf16'], 0), head)).strip()
    return 'G %s %s ; %s' % (name or '%s_%s' % (case.name, form), head, ' ; '.join(jobs))


# ---- the float64 reference ----
def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


# Two of them are weaker than their names: `tile1_at_bn0` models the dropped bn offset on the cell state only (not on the gate or
# weight columns, where it would be a wrong n0 that every other check sees), and `koff_shift` on a job whose K is wider than its
# segments (the plain rider) reads NaN columns of Bt: it is rejected as non-finite, not by the bound.
MUTANTS = ('drop_tile', 'double_tile', 'koff_shift', 'swap_rows', 'cprev_ungathered', 'slot_off', 'not_skipped', 'cprev_not_skipped', 'swap_f_o',
           'tile1_at_bn0')


class Ref:
    pass


def reference(case, job, step, mutant=None, dtype=np.float64, sel=None):
    """What the job must give at `step`: gather, concatenate by koff, multiply in float64, add bias and zinit, then the cell exactly
    as tests/test_gpu_activations.py::test_lstm_cell_within_bound_of_float64 states it.  mutant: one wrong reading of the arguments;
    None is returned where it does not apply to the job at this step.  dtype float32: the same in float32 arithmetic (to show that
    the comparator's bounds are not tighter than float32 itself).  sel: the rows to compute (an index array; default: all)."""
    M, lstm = job.M, case.lstm(job)
    sel = np.arange(M) if sel is None else sel
    r = Ref()
    r.live = job.live()[sel]
    Bt_all = job.Bt.astype(np.float64)
    Bt = np.where(job.covered(), Bt_all, 0.0)
    A = np.zeros((M, job.Ktot))
    read, active = [], []
    for i, sg in enumerate(job.segs):
        m = None
        if mutant == 'swap_rows' and sg.rows is not None and not (step == 0 and sg.first is not None) and 'swap_rows' not in read:
            m = 'swap_rows'
        if mutant == 'slot_off' and not (step == 0 and (sg.first is not None or sg.skip_first)) and 'slot_off' not in read:
            m = 'slot_off'
        if mutant == 'not_skipped' and step == 0 and sg.skip_first and sg.first is None:
            m = 'not_skipped'
        if m:
            read.append(m)
        a = sg.read(step, M, m)
        if a is not None:
            assert not A[:, sg.koff:sg.koff + sg.width].any(), 'segments overlap in K'
            A[:, sg.koff:sg.koff + sg.width] = a
            active.append((sg, a[sel]))
    if mutant in ('swap_rows', 'slot_off', 'not_skipped') and mutant not in read:
        return None
    A = A[sel]
    with np.errstate(invalid='ignore'):
        if dtype == np.float32:
            z = (A.astype(np.float32) @ Bt.astype(np.float32).T).astype(np.float64)
        else:
            z = A @ Bt.T
        mag = np.abs(A) @ np.abs(Bt).T
        if mutant in ('drop_tile', 'double_tile', 'koff_shift'):
            if not active:
                return None
            sg, a = active[-1]
            if mutant == 'koff_shift':      # the last segment's weights read 16 columns off
                k2 = sg.koff + 16 if sg.koff + 16 + sg.width <= job.Ktot else sg.koff - 16
                if k2 < 0:
                    return None
                z = z - a @ Bt[:, sg.koff:sg.koff + sg.width].T + a @ Bt_all[:, k2:k2 + sg.width].T
            else:                           # its second 16-wide K tile dropped / counted twice
                t = a[:, 16:32] @ Bt[:, sg.koff + 16:sg.koff + 32].T
                z = z - t if mutant == 'drop_tile' else z + t
    for extra in ([job.bias] if job.bias is not None else []) + ([job.zinit.read(step, M)[sel]] if job.zinit is not None else []):
        z = (z.astype(dtype) + extra.astype(dtype)).astype(np.float64)
        mag = mag + np.abs(extra)
    r.z, r.mag = z, mag
    if not lstm:
        return None if mutant in ('cprev_ungathered', 'cprev_not_skipped', 'swap_f_o', 'tile1_at_bn0') else r
    U = job.N // GATES
    cols = gate_columns(U)
    cm = None
    if mutant == 'cprev_ungathered':
        if job.c_in.rows is None or (step == 0 and (job.c_in.first is not None or job.c_in.skip_first)):
            return None
        cm = 'ungathered'
    if mutant == 'cprev_not_skipped':       # the zero state of step 0 read from the pool instead
        if not (step == 0 and job.c_in.skip_first and job.c_in.first is None):
            return None
        cm = 'not_skipped'
    cp = job.c_in.read(step, M, cm)
    cp = np.zeros((len(sel), U)) if cp is None else cp[sel]
    if mutant == 'tile1_at_bn0':            # the cell state of column tile 1 read at bn = 0
        if not cp[r.live].any():
            return None
        cp = cp.copy()
        cp[:, BLOCK:2 * BLOCK] = cp[:, :BLOCK]
    if mutant == 'swap_f_o':
        cols = cols[[0, 3, 2, 1]]
    zi, zf, zg, zo = (z[:, cols[g]].astype(dtype) for g in range(GATES))
    cpd = cp.astype(dtype)
    with np.errstate(invalid='ignore', over='ignore'):
        i, f, g, o = _sigmoid(zi), _sigmoid(zf), np.tanh(zg), _sigmoid(zo)
        c = f * cpd + i * g
        h = o * np.tanh(c)
    r.cprev, r.i, r.f, r.g, r.o = cp, *(v.astype(np.float64) for v in (i, f, g, o))
    r.c, r.h = c.astype(np.float64), h.astype(np.float64)
    r.gates = np.empty((len(sel), job.N))
    for k, v in enumerate((r.i, r.f, r.g, r.o)):
        r.gates[:, gate_columns(U)[k]] = v
    # ez: what an error of MAX_BOUND units in a pre-activation is, the largest of the unit's four gates
    r.ez = (MAX_BOUND * EPS * mag)[:, gate_columns(U)].max(axis=1)
    return r


# ---- the comparator ----
# Every number is the project's: RMS_BOUND / MAX_BOUND (tests/test_gpu_gemm.py: error of a contraction in units of 2^-24 sum|a||b|,
# applied there to both arithmetics), ACT_BOUND and the cell's own bound bc (tests/test_gpu_activations.py).
#
# Plain jobs: rms and max of (got - z) / (2^-24 (sum|a||b| + |bias|)) over the live rows under RMS_BOUND and MAX_BOUND.
#
# Cell outputs, element by element.  The kernel's pre-activations are off by at most ez = MAX_BOUND 2^-24 (sum|a||b| + |bias| +
# |zinit|) (the largest of the unit's four gates), and the cell on exact pre-activations is within bc = ACT_BOUND (|c_prev| + 2) +
# 2 2^-24 (|f c_prev| + |i g|) + 1e-12 of c (test_lstm_cell_within_bound_of_float64).  To first order in ez (ez < 1e-5 here, and the
# second derivatives of sigmoid and tanh are below 1: the second-order term is below 1e-10 ez),
#   c = f c_prev + i g:  |dc/dz_f| = |sigmoid' c_prev| <= |c_prev| / 4,  |dc/dz_i| = |sigmoid' g| <= 1/4,  |dc/dz_g| = |i tanh'| <= 1
#       bc' = bc + ez (|c_prev| / 4 + 1/4 + 1)
#   h = o tanh(c):  both activations (2 ACT_BOUND), the error of c (|tanh'| <= 1, o <= 1), |dh/dz_o| = |sigmoid' tanh c| <= 1/4, one rounding
#       bh' = 2 ACT_BOUND + bc' + ez / 4 + 2 2^-24 |h|
# Activated gates: ACT_BOUND + ez / 4 (sigmoid' <= 1/4), ACT_BOUND + ez for g (tanh' <= 1).
def plain_errors(got, ref):
    """(rms, max) over the live rows in units of 2^-24 sum|a||b|; inf where a live element is not finite"""
    live = ref.live
    if not np.isfinite(got[live]).all():
        return float('inf'), float('inf')
    err = (got[live].astype(np.float64) - ref.z[live]) / (ref.mag[live] * EPS)
    return float(np.sqrt(np.mean(err ** 2))), float(np.abs(err).max())


def cell_bounds(ref):
    cp = np.abs(ref.cprev)
    bc = ACT_BOUND * (cp + 2) + 2 * EPS * (np.abs(ref.f * ref.cprev) + np.abs(ref.i * ref.g)) + 1e-12
    bc = bc + ref.ez * (cp / 4 + 0.25 + 1)
    bh = 2 * ACT_BOUND + bc + ref.ez / 4 + 2 * EPS * np.abs(ref.h)
    return bc, bh


def cell_ratios(c, h, ref):
    """(M, U) error / bound of c and of h; inf where an element is not finite (dead rows: 0)"""
    bc, bh = cell_bounds(ref)
    out = []
    for got, want, bound in ((c, ref.c, bc), (h, ref.h, bh)):
        with np.errstate(invalid='ignore'):
            ratio = np.abs(got.astype(np.float64) - want) / bound
        ratio[~np.isfinite(got)] = np.inf
        ratio[~ref.live] = 0
        out.append(ratio)
    return out


def gate_ratio(gates, ref):
    U = ref.c.shape[1]
    bound = np.empty_like(ref.gates)
    cols = gate_columns(U)
    for k in range(GATES):
        bound[:, cols[k]] = ACT_BOUND + (ref.ez if k == 2 else ref.ez / 4)
    with np.errstate(invalid='ignore'):
        ratio = np.abs(gates.astype(np.float64) - ref.gates) / bound
    ratio[~np.isfinite(gates)] = np.inf
    ratio[~ref.live] = 0
    return ratio


def judge(case, job, ref, out):
    """The figures of one job's outputs `out` (name -> (M, width) of the addressed slot) against `ref`, and whether they pass:
    plain {'rms', 'max'}, cell {'c', 'h'} (+ 'gates'): worst error / bound."""
    if not case.lstm(job):
        rms, mx = plain_errors(out['out'], ref)
        return {'rms': rms, 'max': mx}, rms < RMS_BOUND and mx < MAX_BOUND
    rc, rh = cell_ratios(out['c_out'], out['out'], ref)
    fig = {'c': float(rc.max()), 'h': float(rh.max())}
    if 'gates_out' in out:
        fig['gates'] = float(gate_ratio(out['gates_out'], ref).max())
    return fig, all(v <= 1.0 for v in fig.values())


def outputs_of(case, job, ref):
    """the outputs a launch would give if it computed `ref` (float32, as the kernels store them)"""
    if not case.lstm(job):
        return {'out': ref.z.astype(np.float32)}
    out = {'out': ref.h.astype(np.float32), 'c_out': ref.c.astype(np.float32)}
    if job.gates_out is not None:
        out['gates_out'] = ref.gates.astype(np.float32)
    return out
