"""The forms of the train step's persistent recurrences (csrc/train_plan.h, csrc/train.hip, csrc/train_persist*.hip): a case table that
reaches every instantiation the dispatchers name, the plan restated (grid, train_form), and the two input-level mistakes a persistent
kernel could make that tests/grad_noise_cases.py's mutations do not model.  Loss, norm and every gradient of a case are held to
the float64 oracle by the method and the constants of tests/grad_noise_cases.py (tests/test_gpu_train_forms.py on the device,
tests/test_train_form_cases.py without one).

Lengths.  A case's source length S and target length L count the characters ahead of the end character, as L does in
grad_noise_cases.CASES (there S = L): the encoder runs T = S + 1 steps, the decoder U = L + 2, the last of which never carries
weight; a target of length 0 is the end character alone.  About a third of the source lines are shorter than S, the shortest of
one character (of none where S = 1; grad_noise_cases.build, source=S), and one target line is half as long."""
import numpy as np

from oracle.train import forward_backward
from tests import grad_noise_cases as gn

# ------------------------------------------------------------------------------------------------------------------ the form
# csrc/train_plan.h restated: the C++ is held to this file by tests/test_train_form_cases.py through tests/train_plan_driver.cpp
KINDS = ('rec', 'rec_bwd', 'cell', 'cell_bwd')
ROW_BLOCK = 32                      # rows of a row block: TRAIN_ROW_BLOCK = train_tile.h's BM
CAP = 16                            # persistent launches of one step: TRAIN_LAUNCH_CAP (the gate, rec_abort[], rec_cnt's slots)
MIN_CUS = 64                        # TRAIN_MIN_CUS
# the widths NT = W / 32 with an instantiation (CASV_TRAIN_*_WIDTHS), the workgroups per CU a form plans for, the hand-off counters
# per row block, and the longest source the cell's backward can defer its sums for
NT = {'rec': tuple(range(1, 17)), 'rec_bwd': (4, 8, 12, 16), 'cell': (4, 8, 16), 'cell_bwd': (4, 8, 16)}
BLOCKS_PER_CU = {'rec': 2, 'rec_bwd': 2, 'cell': 1, 'cell_bwd': 1}
COUNTERS = {'rec': 2, 'rec_bwd': 16, 'cell': 3, 'cell_bwd': 12}
DEFER_MAX_T = 288
KERNEL = {'rec': 'train_recurrence_kernel', 'rec_bwd': 'train_recurrence_bwd_kernel', 'cell': 'train_attention_cell_kernel',
          'cell_bwd': 'train_attention_cell_bwd_kernel'}
SPLIT_KERNEL = 'train_attention_cell_bwd_rows_kernel'       # the cell's backward split: a second launch beside the first (same NT)


def counter_bytes(kind, B):
    """A launch's hand-off counters: 32 words each, then 32 words the first of which is the give-up word."""
    return (COUNTERS[kind] * ((B + ROW_BLOCK - 1) // ROW_BLOCK) * 32 + 32) * 4


def slot_bytes(B):
    """The slot a launch takes, whatever its kind: the largest kind's counters."""
    return max(counter_bytes(kind, B) for kind in KINDS)


def grid(kind, W, C, B, jobs, cus, per_cu, U=1):
    """The workgroups of a launch, or 0 where the shape has no persistent form on `cus` CUs: train_plan.h's train_form_grid."""
    cell = kind in ('cell', 'cell_bwd')
    if B < 1 or W < 32 or W % 32:
        return 0
    if kind in ('rec_bwd', 'cell_bwd') and W % 128:
        return 0
    if cell and (W != C or U < 1):
        return 0
    if not cell and jobs not in (1, 2):
        return 0
    if kind == 'cell_bwd' and C > 1024:
        return 0
    if W // 32 not in NT[kind]:
        return 0
    n = (1 if cell else jobs) * ((B + ROW_BLOCK - 1) // ROW_BLOCK) * (W // 32)
    return n if n <= per_cu * cus else 0


def sites(cfg, T, U):
    """The places of a step that can take a persistent launch, in train.hip's order: (kind, layers, lengths)."""
    D = cfg.depth
    deep = bool(cfg.deep_bidirectional_encoder) and D >= 2
    pair1 = (('enc1_fw', 'enc1_bw'), (T, T))
    out = [('rec',) + pair1]
    for n in range(2, D + 1):           # encoder layer n beside decoder layer n - 1 (deep: the two directions pair, the decoder walks alone)
        if deep:
            out += [('rec', ('enc%d_fw' % n, 'enc%d_bw' % n), (T, T)), ('rec', ('dec%d' % (n - 1),), (U,))]
        else:
            out.append(('rec', ('enc%d' % n, 'dec%d' % (n - 1)), (T, U)))
    out += [('cell', ('dec%d' % D,), (U,)), ('cell_bwd', ('dec%d' % D,), (U,))]
    for n in range(D - 1, 0, -1):
        if deep:
            out += [('rec_bwd', ('dec%d' % n,), (U,)), ('rec_bwd', ('enc%d_fw' % (n + 1), 'enc%d_bw' % (n + 1)), (T, T))]
        else:
            out.append(('rec_bwd', ('dec%d' % n, 'enc%d' % (n + 1)), (U, T)))
    return out + [('rec_bwd',) + pair1]


def train_form(cfg, B, T, U, cus=256, blocks_per_cu=(2, 2, 1, 1), persistent=True, deterministic=False, backoff=False,
               not_plain=(), defer=1, split=True, split_off=False, rows_fit=True):
    """The form of one mode-1 / mode-2 step, restated from train_plan.h's TrainStepPlan asked at the sites of train.hip
    (layers_forward, layers_backward, forward_cell, cell_backward_persistent) in the step's order.
    The gate: option "persistent" != 0, "deterministic" off, no back-off pending, MIN_CUS CUs.  not_plain: the kinds whose sites' own
    condition fails (rec_bwd: a job's kr != W; cell: hs_ld != W).  defer / split: CASV_ATTN_DEFER and CASV_TOPB_SPLIT (after the
    serialised-dispatch rule); split_off: a step gave up in the two-launch form; rows_fit: both launches fit a CU.
    -> dict(launches = per site dict(kind, kernel, NT, jobs, layers, lengths, grid, persistent, split, capped, slot, offset, counters,
    defer, site), count = the persistent launches of the step after the cap CAP (the statistic "train_persistent_launches"),
    capped = the layers of the sites whose shape has a persistent form but which come behind the CAP-th launch and run per step).
    split: the attention cell's backward takes its two-launch form (SPLIT_KERNEL beside the main kernel: one launch of the count).
    slot / offset / counters: the launch's slot of the counter buffer, its byte offset, and its kind's counter bytes, behind which its
    give-up word sits.  site: the plan's inputs for the site, as tests/train_plan_driver.cpp reads them."""
    W, C = cfg.width, cfg.ctx_width
    per_cu = dict(zip(KINDS, blocks_per_cu))
    gate = bool(persistent) and not deterministic and not backoff and cus >= MIN_CUS
    launches, count, capped = [], 0, []
    for kind, layers, lengths in sites(cfg, T, U):
        plain = kind not in not_plain
        steps = max(lengths)
        g = grid(kind, W, C, B, len(layers), cus, per_cu[kind], steps) if gate and plain else 0
        on = g > 0 and count < CAP
        if g > 0 and not on:
            capped.append(layers)
        ln = dict(kind=kind, kernel=KERNEL[kind], NT=W // 32, jobs=len(layers), layers=layers, lengths=lengths, grid=g,
                  persistent=on, split=False, capped=g > 0 and not on, slot=0, offset=0, counters=0, defer=0,
                  site=(kind, W, C, B, steps, len(layers), per_cu[kind], int(plain), T, defer, int(split), int(split_off), int(rows_fit)))
        if on:
            ln.update(slot=count, offset=count * slot_bytes(B), counters=counter_bytes(kind, B))
            if kind == 'cell_bwd':
                ln.update(defer=defer if T <= DEFER_MAX_T and W % 64 == 0 and C % 64 == 0 else 0, split=bool(split and not split_off and rows_fit))
        count += on
        launches.append(ln)
    return dict(launches=launches, count=count, capped=capped, slot_bytes=slot_bytes(B),
                gate=(int(bool(persistent)), int(deterministic), int(backoff), cus))


def driver_lines(name, f):
    """A step of train_form as tests/train_plan_driver.cpp reads it ..."""
    return ['S %s %d %d %d %d %d' % ((name,) + f['gate'] + (len(f['launches']),))] + \
           ['%s %d %d %d %d %d %d %d %d %d %d %d %d' % ln['site'] for ln in f['launches']]


def records(f):
    """... and as it prints it: one record per site, then the step's count."""
    return ['site kind=%s persistent=%d capped=%d grid=%d nt=%d slot=%d offset=%d counters=%d defer=%d split=%d'
            % (ln['kind'], ln['persistent'], ln['capped'], ln['grid'], ln['NT'] if ln['grid'] else 0, ln['slot'], ln['offset'], ln['counters'],
               ln['defer'], ln['split']) for ln in f['launches']] + ['step count=%d slot_bytes=%d' % (f['count'], f['slot_bytes'])]


# ------------------------------------------------------------------------------------------------------------------ the cases
def _case(name, d, W, B, S, L, count, masks=True, flags=None, A=1, frozen=(), V=40):
    """((name, d, W, V, B, L, emb_scale, masks, flags, alternatives, frozen) as in grad_noise_cases.CASES, S, predicted launches)."""
    return ((name, d, W, V, B, L, 4.0, masks, dict(flags or {}), A, tuple(frozen)), S, count)


def _width_count(W):       # depth 2: two forward recurrences; whole column tiles of 128: two backward ones; 128, 256, 512: the cell's two
    return 2 + (2 if W % 128 == 0 else 0) + (2 if W // 32 in NT['cell'] and W % 128 == 0 else 0)


# Every forward NT 1 .. 16, backward NT 4, 8, 12, 16, the cell and its backward at 4, 8, 16; elsewhere the per-step backward
# (gemm_bwd.hip on the fused path) behind a persistent forward pass.  B = 33: two row blocks, the second of one row.
WIDTHS = [_case('w%d' % W, 2, W, 33, 4, 9, _width_count(W)) for W in range(32, 513, 32)]
# Row-block edges at 8 (W = 128), 4 (W = 256) and 2 (W = 512: two waves per row) rows per workgroup
ROWS = [_case('w128_b%d' % B, 2, 128, B, 4, 9, 6) for B in (1, 31, 32, 33, 64, 65)]
ROWS += [_case('w512_b%d' % B, 2, 512, B, 4, 9, 6) for B in (1, 2, 33)]
ROWS += [_case('w256_b%d' % B, 2, 256, B, 4, 9, 6) for B in (4, 5)]
# Two-job launches of unequal lengths, either job the longer one by many steps, and the shortest jobs there are (T = U = 2)
LENGTHS = [_case('s%d_l%d' % (S, L), 2, 128, 5, S, L, 6) for S, L in ((1, 0), (1, 11), (12, 1), (40, 2), (2, 40))]
LENGTHS += [_case('d3_s3_l20', 3, 128, 5, 3, 20, 8)]        # both pairs (enc3, dec2) and (enc2, dec1) of unequal lengths
# depth 1: C = 2W, the cell per step, layer 1's pair alone persistent.  depth 8: 2 x 8 + 2 = 18 places, the cap of 16 is reached in
# the backward pass: (dec1, enc2) and (enc1_fw, enc1_bw) walk backwards per step behind the sixteen persistent launches before them.
DEPTH = [_case('d1', 1, 128, 5, 4, 9, 2), _case('d3', 3, 128, 5, 4, 9, 8), _case('d8_plain', 8, 128, 5, 4, 9, 16, masks=False)]
DEPTH8_CAPPED = [('dec1', 'enc2'), ('enc1_fw', 'enc1_bw')]
TOPOLOGIES = [_case('residual_d4', 4, 128, 33, 4, 9, 10, flags=dict(residual_connections=True)),
              _case('bridge_d2', 2, 128, 33, 4, 9, 6, flags=dict(bridge_dense=True)),
              # (C = 2W: the cell per step; the decoder layer walks alone: one-job launches of both recurrences)
              _case('deep_d2', 2, 128, 33, 4, 9, 6, flags=dict(deep_bidirectional_encoder=True)),
              _case('frozen_d3', 3, 128, 33, 4, 9, 8, frozen=('enc1_', 'dec1_')),
              _case('confusion_d2', 2, 128, 33, 4, 9, 6, A=2)]
# 256 CUs: 2 jobs x 32 row blocks x 8 = 512 = 2 x 256 workgroups and 32 x 8 = 256 for the cell -- the last batch with a persistent
# form; one line more is a 33rd row block, no grid fits and the whole step is per step
RESIDENCY = [_case('w256_b1024', 2, 256, 1024, 2, 1, 6), _case('w256_b1025', 2, 256, 1025, 2, 1, 0)]
ALL = WIDTHS + ROWS + LENGTHS + DEPTH + TOPOLOGIES + RESIDENCY
IDS = [c[0][0] for c in ALL]
BY_NAME = {c[0][0]: c for c in ALL}
# the cases whose bounds are shown to fail on a mistake (tests/test_train_form_cases.py): a width, a row-block edge, unequal lengths
# (T > U), the capped depth and the residual topology
MUTATED = ('w96', 'w128_b33', 's12_l1', 'd8_plain', 'residual_d4')


def build(fc):
    """grad_noise_cases.build of a case: source lines of its S characters, ragged."""
    return gn.build(fc[0], source=fc[1])


def form(fc, cus=256, persistent=True, **inputs):
    """train_form of a case's step."""
    (name, d, W, V, B, L, es, mk, flags, A, frozen), S, _ = fc
    from oracle import ModelConfig
    return train_form(ModelConfig(depth=d, width=W, voc_size=V, **flags), B, S + 1, L + 2, cus=cus, persistent=persistent, **inputs)


_ORACLES, _EVALS = {}, {}


def oracles(fc):
    """(cfg, w, inputs, batch, o64, o32) of a case, computed once per process and left as they are."""
    name = fc[0][0]
    if name not in _ORACLES:
        cfg, w, inputs, batch = build(fc)
        frozen = fc[0][10]
        _ORACLES[name] = (cfg, w, inputs, batch, gn.oracle(cfg, w, inputs, np.float64, frozen), gn.oracle(cfg, w, inputs, np.float32, frozen))
    return _ORACLES[name]


def eval_losses(fc):
    """(float64, float32) loss_ce of the oracle's mask-free evaluation of a case, computed once per process."""
    name = fc[0][0]
    if name not in _EVALS:
        cfg, w, inputs = oracles(fc)[:3]
        _EVALS[name] = (eval_loss(cfg, w, inputs, np.float64), eval_loss(cfg, w, inputs, np.float32))
    return _EVALS[name]


def eval_loss(cfg, w, inputs, dtype):
    """The oracle's loss_ce of a mode-0 evaluation: no masks, no regulariser."""
    enc_in, dec_in, dec_out, wts, _ = inputs
    cast = lambda a: np.asarray(a, dtype)
    _, _, aux = forward_backward(cfg, {k: cast(v) for k, v in w.items()}, cast(enc_in), cast(dec_in), cast(dec_out), cast(wts), None,
                                 want_grads=False, window_dtype=np.float32)
    return float(aux['loss_ce'])


def scalar_ratio(got, a32, r64):
    """|got - r64| in units of |a32 - r64|, the unit floored at 2^-24 x |r64| (grad_noise_cases.ratios on one number)."""
    return abs(got - r64) / max(abs(a32 - r64), 2.0 ** -24 * max(abs(r64), 1e-30))


def floored_units(o32, o64):
    """The quantities of a case whose noise unit max|o32 - o64| sits on the floor 2^-24 x max|o64| -- the fp32 oracle is then right
    to half a unit in the last place of the tensor's largest entry everywhere, and a ratio counts those half units instead of the
    oracle's noise -- and how many quantities there are.  (The rms unit is no measure of this: rms(o32 - o64) of a weight
    gradient is routinely below that floor, 0.1 to 0.6 of it in grad_noise_cases.CASES as here, because most entries of such a
    tensor are far smaller than its largest.)"""
    items = [('loss', o32[0], o64[0]), ('norm', o32[1], o64[1])] + [(k, o32[2][k], o64[2][k]) for k in sorted(o64[2])]
    on = []
    for k, a, r in items:
        a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
        if float(np.abs(a - r).max()) <= 2.0 ** -24 * max(float(np.abs(r).max()), 1e-30):
            on.append(k)
    return on, len(items)


def form_mutations(cfg, w, inputs, frozen=()):
    """{name: float64 oracle (loss, norm, grads)} of the two mistakes of a persistent launch's edges:
    row_clamp_leaks       the last row's source is the row's before it (a clamped row index that is stored after all)
    shorter_job_cut       the shorter job of the (encoder n, decoder n - 1) pairs loses its last step: where T < U the last source
                          position of every line is a zero row; where U < T every line's target step U - 2 is removed -- the last
                          step that can carry weight (step U - 1 carries none in any line and feeds nothing: no output sees it)."""
    enc_in, dec_in, dec_out, wts, masks = inputs
    (B, U), T = np.asarray(wts).shape, np.asarray(enc_in).shape[1]
    e1 = np.array(enc_in, copy=True); e1[B - 1] = e1[B - 2]
    out = {'row_clamp_leaks': gn.oracle(cfg, w, (e1, dec_in, dec_out, wts, masks), np.float64, frozen)}
    if T < U:
        e2 = np.array(enc_in, copy=True); e2[:, T - 1] = 0
        out['shorter_job_cut'] = gn.oracle(cfg, w, (e2, dec_in, dec_out, wts, masks), np.float64, frozen)
    elif U < T:
        w2 = np.array(wts, copy=True); w2[:, U - 2] = 0
        do = np.array(dec_out, copy=True); do[:, U - 2] = 0
        out['shorter_job_cut'] = gn.oracle(cfg, w, (enc_in, dec_in, do, w2, masks), np.float64, frozen)
    return out
