"""One backward time step of an LSTM layer, per pipeline path: the cases, a float64 reference, a float32 restatement with named
wrong readings, and the comparator (no GPU here).

tests/test_gpu_bwd_step.py runs every case through casv_debug_bwd_step in both forms -- 0: the fused launch of csrc/gemm_bwd.hip
(lstm_bwd_gemm_kernel), 1: lstm_bwd_kernel followed by the plain GEMM -- and judges what comes back with `judge`;
tests/test_bwd_step_cases.py holds this module itself: the restated launch plan against csrc/train_plan.h, the table's reach, the
restatement under the comparator, every wrong reading caught.

The step (oracle/train.py lstm_backward, csrc/train_kernels.hip lstm_bwd_kernel), per row r and unit u:
    dh  = a * mask_a + b + c                     (each part optional)
    tc  = tanh(cell);  dct = dh * o * (1 - tc^2) + dc_in
    dz_i = dct * g * i * (1 - i)    dz_f = dct * c_prev * f * (1 - f)    dz_g = dct * i * (1 - g^2)    dz_o = dh * tc * o * (1 - o)
    dc  = dct * f                                out = dz . Bt^T
with gates and dz in the interleaved column order [unit / 32][gate i, f, g, o][unit % 32], which is also Bt's K order.

The comparator has two stages, so that a pointwise error and a GEMM error cannot hide each other.
  1. dz and dc against float64, element by element, in units of 2^-24 x the MAGNITUDE of the expression: the same expression with
     every term and factor replaced by its absolute value and every difference by a sum (|a mask| + |b| + |c| for dh, 1 + tc^2 for
     1 - tc^2, |dh| o (1 + tc^2) + |dc_in| for dct, 1 + |i| for 1 - i, ...), so that cancellation in dh, in dct or in 1 - tc^2
     does not shrink the unit.  The bound is 4 E_PW, where E_PW is the largest error of the float32 restatement below (IEEE float32
     products and sums in the kernel's order around a correctly rounded tanh) in these units over the whole table: the margin
     tests/test_gpu_score.py gives its float32 head, for the same reason -- the device has another tanhf and contracts the same
     formula differently.  E_PW is recorded here and in profiles/bwd_step_noise.txt; the CPU test measures it again.
  2. out against the float64 product of the dz THAT CAME BACK with Bt, in units of 2^-24 sum|dz||Bt|, under the GEMM tests' own
     RMS_BOUND / MAX_BOUND (tests/test_gpu_gemm.py).  One 32-k stage dropped or doubled is >= 1e3 of these units.
  Exact: where a magnitude is 0 the value is +-0; nothing is stored outside rows < rows, columns < N (the 0xFF bytes the entry
  filled the outputs with are still there); every result is finite but on a row whose `a` is NaN, which is NaN throughout."""
import numpy as np

from tests.test_gpu_gemm import MAX_BOUND, RMS_BOUND

EPS = 2.0 ** -24
UNTOUCHED = np.uint32(0xFFFFFFFF)
# The float32 restatement's largest pointwise error over ALL, in the units of stage 1 (test_bwd_step_cases.py measures it:
# test_the_restatement_passes_and_the_recorded_noise_is_what_it_measures); the device's bound is PW_MARGIN times this.
E_PW = 3.817
PW_MARGIN = 4.0


# ------------------------------------------------------------------------------------------------------------------ the launch plan
def plan(jobs_rows_n, W):
    """csrc/train_plan.h, bwd_step_plan, restated: (blocks, ksplit, gper) of the fused launch for [(rows, N), ...] jobs of width W.
    Workgroups of 32 rows x 128 columns, the grid the larger job's; the most K shares <= 8 that divide the W / 32 unit groups and
    keep jobs x blocks x shares <= 640."""
    blocks = max(-(-rows // 32) * -(-n // 128) for rows, n in jobs_rows_n)
    groups = W // 32
    ksplit = max([s for s in range(2, min(groups, 8) + 1) if groups % s == 0 and blocks * len(jobs_rows_n) * s <= 640] or [1])
    return blocks, ksplit, groups // ksplit


# ------------------------------------------------------------------------------------------------------------------ jobs and cases
class Job:
    """One layer's step, as casv_debug_bwd_step takes it (engine.debug_bwd_step).  a / b / c / c_prev: None or (rows, W) float32
    column windows of wider arrays (the row stride is the ld)."""
    def __init__(self, rows, W, N, ld_out=None):
        self.rows, self.W, self.N, self.ld_out = rows, W, N, N if ld_out is None else ld_out
        self.a = self.mask_a = self.b = self.c = self.c_prev = None
        self.nan_rows = []


class Case:
    def __init__(self, name, jobs, forms=(0, 1)):
        self.name, self.jobs, self.forms = name, jobs, forms
        self.W = jobs[0].W
        self.plan = plan([(j.rows, j.N) for j in jobs], self.W)


def _gates(rng, rows, W):
    """[rows][4W] interleaved: i, f, o in (0.05, 0.95), g in (-0.95, 0.95)"""
    g = rng.uniform(0.05, 0.95, (rows, W // 32, 4, 32))
    g[:, :, 2] = rng.uniform(-0.95, 0.95, (rows, W // 32, 32))
    return g.reshape(rows, 4 * W).astype(np.float32)


def make_job(seed, rows, W, N=None, a='plain', mask=True, b='plain', c=False, c_prev='plain', ld_out=None, ld_cprev=None, ctx=0,
             values=None):
    """a: 'plain' (lda = W), 'wide' (the second half of a 2W-wide row) or None; mask: per-unit dropout mask with dropped units;
    b: 'plain', 'top' (columns ctx .. ctx + W of a row of ctx + W: the attention cell's dRec) or None; c: the query path's part;
    c_prev: 'plain', None, or ld_cprev > W.  values: 'gates_exact', 'cell_saturated', 'zero_rows', ('nan_row', r)."""
    rng = np.random.default_rng(seed)
    N = W if N is None else N
    job = Job(rows, W, N, ld_out)
    f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    if a == 'plain':
        job.a = f32(rng.standard_normal((rows, W)))
    elif a == 'wide':
        job.a = f32(rng.standard_normal((rows, 2 * W)))[:, W:]
    if mask:
        assert job.a is not None
        job.mask_a = f32((rng.random(W) >= 0.25) / 0.75)
        job.mask_a[3] = 0.0
    if b == 'plain':
        job.b = f32(rng.standard_normal((rows, W)))
    elif b == 'top':
        job.b = f32(rng.standard_normal((rows, ctx + W)))[:, ctx:]
    if c:
        job.c = f32(rng.standard_normal((rows, W)) * 0.5)
    if c_prev == 'plain':
        ld = W if ld_cprev is None else ld_cprev
        job.c_prev = f32(rng.standard_normal((rows, ld)) * 1.5)[:, :W]
    job.gates = _gates(rng, rows, W)
    job.cell = f32(rng.standard_normal((rows, W)) * 1.5)
    job.dc_in = f32(rng.standard_normal((rows, W)))
    job.Bt = f32(rng.standard_normal((N, 4 * W)) / np.sqrt(4 * W))
    kind = values[0] if isinstance(values, tuple) else values
    if kind == 'gates_exact':          # sigmoids at exactly 0 and 1, tanh at exactly -1, 0 and 1: a third of the entries each way
        g = job.gates.reshape(rows, W // 32, 4, 32)
        pick = rng.integers(0, 3, g.shape)
        g[pick == 0] = 0.0
        g[pick == 1] = 1.0
        g[:, :, 2][rng.integers(0, 4, g[:, :, 2].shape) == 0] = -1.0
    elif kind == 'cell_saturated':     # tanhf is +-1 from |x| of about 9.1 on; around the threshold and far beyond it
        sat = rng.random((rows, W)) < 0.5
        job.cell[sat] = (rng.choice([-1.0, 1.0], sat.sum()) * rng.choice([8.5, 9.0, 9.25, 12.0, 30.0, 88.0], sat.sum())).astype(np.float32)
    elif kind == 'zero_rows':          # rows that receive no gradient at all: dz and dc exactly 0
        for arr in (job.a, job.b, job.c, job.dc_in):
            if arr is not None:
                arr[1::4] = 0.0
    elif kind == 'nan_row':
        job.a[values[1]] = np.nan
        job.nan_rows = [values[1]]
    return job


def build_cases():
    """{name: Case}.  Names: g<gper>_... the pipeline paths; <input form>_w<width>; values; two-job and stride cases."""
    cases = []

    def case(name, *jobs, forms=(0, 1)):
        cases.append(Case(name, list(jobs), forms))
    mj = make_job
    # gper 1: the prologue and the last group alone
    case('g1_w32_n32', mj(1, 5, 32, 32))
    case('g1_w32_n96', mj(2, 33, 32, 96))
    case('g1_w64', mj(3, 31, 64))
    case('g1_w96', mj(4, 32, 96))
    case('g1_w160', mj(5, 65, 160))
    case('g1_w256', mj(6, 33, 256))
    case('g1_w32_one_row', mj(7, 1, 32, 32))
    # gper 2: one group with its pointwise work, then the last; with K shares and with the plain store
    case('g2_w320', mj(8, 33, 320))
    case('g2_plain_store', mj(9, 5152, 64), mj(10, 5152, 64))
    # gper 3: the loop runs zero times
    case('g3_w288_one_job', mj(11, 33, 288))
    case('g3_w288_two_jobs', mj(12, 65, 288), mj(13, 31, 288))
    case('g3_plain_store', mj(14, 3456, 96), mj(15, 3456, 96))
    # gper 4, 5, 11: the loop runs once, twice, eight times (the last with the plain store)
    case('g4_w640', mj(16, 5, 640))
    case('g5_w800', mj(17, 33, 800))
    case('g11_w352', mj(18, 65, 352))
    # the input forms the train step produces, at one unit group per share and on the looped pipeline
    for W, rows in ((96, 31), (352, 33)):
        case('last_step_w%d' % W, mj(20 + W, rows, W, b=None))
        case('no_a_w%d' % W, mj(21 + W, rows, W, a=None, mask=False))
        case('top_last_step_w%d' % W, mj(22 + W, rows, W, N=2 * W, mask=False, b=None))
    for W, rows in ((96, 33), (288, 32)):
        case('first_step_w%d' % W, mj(23 + W, rows, W, c_prev=None))
        case('a_wide_w%d' % W, mj(24 + W, rows, W, a='wide'))
    for W, rows in ((64, 33), (288, 5)):
        case('top_c1_w%d' % W, mj(25 + W, rows, W, N=2 * W, mask=False, b='top', ctx=W, c=True))
    for W, rows in ((32, 65), (288, 31)):
        case('top_c2_w%d' % W, mj(26 + W, rows, W, N=3 * W, mask=False, b='top', ctx=2 * W, c=True))
    # two jobs of different rows and N: the grid is the larger job's, the smaller job's surplus workgroups leave
    case('two_jobs_uneven', mj(40, 5, 96, 96), mj(41, 37, 96, 160))
    # strides: ld_out > N, ld_cprev > W
    case('strides_w96', mj(42, 31, 96, 100, ld_out=104, ld_cprev=132))
    case('strides_w288', mj(43, 33, 288, ld_out=292, ld_cprev=576))
    # values
    for W, rows in ((64, 33), (352, 31)):
        case('gates_exact_w%d' % W, mj(50 + W, rows, W, values='gates_exact'))
    for W, rows in ((64, 32), (288, 33)):
        case('cell_saturated_w%d' % W, mj(51 + W, rows, W, values='cell_saturated'))
        case('zero_rows_w%d' % W, mj(52 + W, rows, W, c=True, values='zero_rows'))
    case('nan_row_w96', mj(60, 33, 96, values=('nan_row', 7)))
    case('nan_row_w288', mj(61, 65, 288, values=('nan_row', 32)))
    # lstm_bwd_kernel's grid-stride loop takes a second pass from rows * W > 4096 * 256 on: the two-launch form only
    case('grid_stride', mj(70, 4100, 256, 128), forms=(1,))
    return {c.name: c for c in cases}


# ------------------------------------------------------------------------------------------------------------------ the step
def _split(x):
    """(rows, 4W) interleaved -> four (rows, W) arrays i, f, g, o"""
    rows, K = x.shape
    v = x.reshape(rows, K // 128, 4, 32)
    return [v[:, :, k].reshape(rows, K // 4) for k in range(4)]


def _join(parts):
    rows, W = parts[0].shape
    return np.stack([p.reshape(rows, W // 32, 32) for p in parts], axis=2).reshape(rows, 4 * W)


def _absent(job, dt):
    return np.zeros((job.rows, job.W), dt)


def reference(job):
    """The step in float64 by the definition: dict dz (rows, 4W), dc (rows, W), and the magnitudes mz, mc of the same shapes (the
    module's docstring, stage 1)."""
    f8 = lambda x: _absent(job, np.float64) if x is None else np.asarray(x, np.float64)
    a, b, c, cp, cell, dc_in = f8(job.a), f8(job.b), f8(job.c), f8(job.c_prev), f8(job.cell), f8(job.dc_in)
    mask = np.ones(job.W) if job.mask_a is None else job.mask_a.astype(np.float64)
    i, f, g, o = _split(job.gates.astype(np.float64))
    with np.errstate(invalid='ignore'):
        dh = a * mask + b + c
        mdh = np.abs(a * mask) + np.abs(b) + np.abs(c)
        tc = np.tanh(cell)
        dct = dh * o * (1 - tc * tc) + dc_in
        mdct = mdh * np.abs(o) * (1 + tc * tc) + np.abs(dc_in)
        dz = _join([dct * g * i * (1 - i), dct * cp * f * (1 - f), dct * i * (1 - g * g), dh * tc * o * (1 - o)])
        mz = _join([mdct * np.abs(g * i) * (1 + np.abs(i)), mdct * np.abs(cp * f) * (1 + np.abs(f)), mdct * np.abs(i) * (1 + g * g),
                    mdh * np.abs(tc * o) * (1 + np.abs(o))])
        return {'dz': dz, 'dc': dct * f, 'mz': mz, 'mc': mdct * np.abs(f)}


WRONG = ('mask_per_row', 'c_ignored', 'cprev_from_cell', 'ldb_as_w', 'gate_order_ifog', 'dc_in_place', 'stage_twice', 'stale_last_group',
         'rows_past_stored')


def _flat_rows(win, W):
    """what a kernel reads that takes the window's row stride for W: row r = W floats from r * W behind the window's first element"""
    rows = win.shape[0]
    base = win.base if win.base is not None else win
    off = (win.__array_interface__['data'][0] - base.__array_interface__['data'][0]) // 4
    return base.ravel()[off:off + rows * W].reshape(rows, W)


def restate(job, wrong=None):
    """The step in float32 numpy, in the kernels' order of operations (tanh correctly rounded: float64's, rounded once), as the
    entry returns it: dict dz (rows + 1, 4W), dc (rows + 1, W), out (rows + 1, ld_out) with 0xFF bytes wherever nothing is stored.
    wrong: one of WRONG -- what a kernel with that fault would return."""
    assert wrong is None or wrong in WRONG
    rows, W, N = job.rows, job.W, job.N
    f4 = lambda x: _absent(job, np.float32) if x is None else np.asarray(x, np.float32)
    one = np.float32(1)
    a, b, c, cell, dc_in = f4(job.a), f4(job.b), f4(job.c), f4(job.cell), f4(job.dc_in)
    cp = f4(job.c_prev)
    if wrong == 'cprev_from_cell' and job.c_prev is None:
        cp = cell
    if wrong == 'ldb_as_w' and job.b is not None:
        b = _flat_rows(job.b, W)
    if wrong == 'c_ignored':
        c = _absent(job, np.float32)
    mask = np.ones(W, np.float32) if job.mask_a is None else job.mask_a
    mask = np.resize(mask, rows)[:, None] if wrong == 'mask_per_row' else mask[None, :]
    gates = _split(job.gates)
    i, f, g, o = [gates[k] for k in ((0, 1, 3, 2) if wrong == 'gate_order_ifog' else (0, 1, 2, 3))]

    def cells(a, b, c, i, f, g, o, cell, cp, dc_in, mask):
        with np.errstate(invalid='ignore'):
            dh = a * mask + b + c
            tc = np.tanh(cell.astype(np.float64)).astype(np.float32)
            dov = dh * tc
            dct = dh * o * (one - tc * tc) + dc_in
            return [dct * g * i * (one - i), dct * cp * f * (one - f), dct * i * (one - g * g), dov * o * (one - o)], dct * f
    z, dc = cells(a, b, c, i, f, g, o, cell, cp, dc_in, mask)
    if wrong == 'dc_in_place':                   # a column tile reads dL/dc where the first tile has already written the new one
        z, _ = cells(a, b, c, i, f, g, o, cell, cp, dc, mask)
    if wrong == 'stale_last_group' and W >= 64:  # the last unit group's cells from the inputs of the group before
        lo, hi = slice(W - 64, W - 32), slice(W - 32, W)
        zs, dcs = cells(*[x[:, lo] for x in (a, b, c, i, f, g, o, cell, cp, dc_in)], mask if mask.shape[1] == 1 else mask[:, lo])
        for k in range(4):
            z[k][:, hi] = zs[k]
        dc[:, hi] = dcs
    dz = _join(z)
    with np.errstate(invalid='ignore'):
        out = dz @ job.Bt.T
        if wrong == 'stage_twice':               # stage 1 (gate f of unit group 0) contracted twice, stage 2 (gate g) never
            out = out + dz[:, 32:64] @ job.Bt[:, 32:64].T - dz[:, 64:96] @ job.Bt[:, 64:96].T
    res = {'dz': np.empty((rows + 1, 4 * W), np.float32), 'dc': np.empty((rows + 1, W), np.float32),
           'out': np.empty((rows + 1, job.ld_out), np.float32)}
    for v in res.values():
        v.view(np.uint32)[:] = UNTOUCHED
    res['dz'][:rows], res['dc'][:rows], res['out'][:rows, :N] = dz, dc, out
    if wrong == 'rows_past_stored':
        res['dc'][rows] = dc[rows - 1]
    return res


# ------------------------------------------------------------------------------------------------------------------ the comparator
def judge(job, ref, got, pw_bound):
    """(figures, failures): figures = {'pw': largest pointwise error of dz / dc in stage-1 units, 'rms' / 'max': of out in stage-2
    units}; failures = a list of what is wrong, empty if the result passes.  pw_bound: E_PW for the restatement, PW_MARGIN * E_PW
    for the device."""
    rows, W, N = job.rows, job.W, job.N
    fail, fig = [], {}
    live = np.ones(rows, bool)
    live[job.nan_rows] = False
    bits = {k: got[k].view(np.uint32) for k in ('dz', 'dc', 'out')}
    # nothing outside the result region
    for k in ('dz', 'dc', 'out'):
        if not (bits[k][rows:] == UNTOUCHED).all():
            fail.append('%s: a store to a row >= rows' % k)
    if not (bits['out'][:rows, N:] == UNTOUCHED).all():
        fail.append('out: a store behind column N - 1')
    dz, dc, out = got['dz'][:rows].astype(np.float64), got['dc'][:rows].astype(np.float64), got['out'][:rows, :N].astype(np.float64)
    # the NaN row is NaN throughout, everything else finite
    for k, v in (('dz', dz), ('dc', dc), ('out', out)):
        if not np.isnan(v[~live]).all():
            fail.append('%s: the row whose a is NaN is not NaN throughout' % k)
        if not np.isfinite(v[live]).all():
            fail.append('%s: a value that is not finite' % k)
    if fail:
        return fig, fail
    # stage 1
    pw = 0.0
    for k, v, want, mag in (('dz', dz, ref['dz'], ref['mz']), ('dc', dc, ref['dc'], ref['mc'])):
        v, want, mag = v[live], want[live], mag[live]
        zero = mag == 0
        if (v[zero] != 0).any():
            fail.append('%s: a value whose magnitude is 0 is not 0' % k)
        err = np.abs(v - want)[~zero] / (EPS * mag[~zero])
        if err.size:
            pw = max(pw, float(err.max()))
            if err.max() > pw_bound:
                at = np.argwhere(~zero)[int(err.argmax())]
                fail.append('%s[%d][%d]: %.3g units > %.3g' % (k, at[0], at[1], err.max(), pw_bound))
    fig['pw'] = pw
    # stage 2: the contraction of the dz that came back
    Bt = job.Bt.astype(np.float64)
    want, mag = dz[live] @ Bt.T, np.abs(dz[live]) @ np.abs(Bt).T
    v, zero = out[live], mag == 0
    if (v[zero] != 0).any():
        fail.append('out: a value whose magnitude is 0 is not 0')
    err = (v - want)[~zero] / (EPS * mag[~zero])
    fig['rms'] = float(np.sqrt(np.mean(err ** 2))) if err.size else 0.0
    fig['max'] = float(np.abs(err).max()) if err.size else 0.0
    if not (fig['rms'] < RMS_BOUND and fig['max'] < MAX_BOUND):
        fail.append('out: rms %.3g max %.3g units, bounds %.3g / %.3g' % (fig['rms'], fig['max'], RMS_BOUND, MAX_BOUND))
    return fig, fail
