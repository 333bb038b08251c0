"""The launch forms of the decode path's persistent kernels (csrc/persist.hip: persist_decode_kernel, persist_encode_kernel;
csrc/persist_split.hip: persist_split_encode_kernel): the plans of csrc/persist_plan.h restated (decoder_form, encoder_form), the
workgroups per CU the runtime admits for the three kernels as read on an MI355X (RESIDENCY), and a case table that reaches every
form the kernels have -- more than one tile, task or row quarter per workgroup, partial last rounds, idle waves, both attention
forms by each of their conditions, the three softmax-statistics forms, depths 1 / 2 / 8, the row-block edges, the LDS edge, and the
encoders' tile limits.  tests/test_persist_form_cases.py holds the C++ plans to the restatement without a device;
tests/test_gpu_persist_forms.py runs every case, asserts the form that ran from the statistics and compares bits and float64.

A case's L counts the source characters ahead of the end character: the encoder runs T = L + 1 positions (6 to 10 in every case
that is not about T itself: width and batch reach a form, length does not).  Line 1 of every batch of three lines or more is cut
to half its length (a ragged batch: zero rows behind the shorter line)."""
import collections

import numpy as np

from tests import decode_noise_cases as dn
from tests.greedy_tie_cases import greedy_form

# ------------------------------------------------------------------------------------------------------------------ the plans
MIN_CUS, MAX_DEPTH = 64, 8                  # persist_plan.h: PERSIST_MIN_CUS, PERSIST_MAX_DEPTH
LDS_LIMIT = 150 * 1024                      # PERSIST_LDS_LIMIT: staged rows of persist.hip's kernels
ROWS_FORCED, ROWS_DEFAULT, OWN_DEFAULT = 4096, 512, 2
ENC_MAX_TILES, SPLIT_MAX_TILES = 8, 4       # PENC_MAXT, PS_MAXT
SPLIT_DEFAULT_ROWS = 256
SPLIT_LDS = 49152                           # persist_split.hip: PS_LDS_BYTES
DEC_REASONS = ('ok', 'off', 'split_arithmetic', 'cus', 'depth', 'lds', 'not_worth')           # PersistDecPlan::Reason, in order
ENC_REASONS = ('ok', 'off', 'cus', 'depth', 'topology', 'lds', 'own', 'not_worth')             # PersistEncPlan::Reason, in order

# Workgroups per CU that hipOccupancyMaxActiveBlocksPerMultiprocessor reports on an MI355X (256 CUs, 160 KB of LDS per CU) for 256
# threads and the dynamic LDS size of the launch, capped at 2 as the hosts cap it -- read through the statistics
# "decoder_persist_per_cu" / "encoder_persist_per_cu" (profiles/persist_form_ratios.txt).  {kernel: {dynamic LDS bytes: figure}}.
# The chain kernels stage 16 rows of lda floats: two workgroups share a CU up to 73 984 bytes (depth 2, width 384), one from 80 128
# (width 416) to the limit; the split kernel's size is fixed.  Both chain kernels gave the same figure at every size.
RESIDENCY = {
    'decode': {12544: 2, 24832: 2, 28928: 2, 49408: 2, 53504: 2, 61696: 2, 67840: 2, 73984: 2, 80128: 1, 98560: 1, 147712: 1},
    'encode': {12544: 2, 16640: 2, 18688: 2, 24832: 2, 33024: 2, 49408: 2, 61696: 2, 67840: 2, 73984: 2, 80128: 1, 98560: 1, 147712: 1},
    'split': {SPLIT_LDS: 2}}


def residency(kernel, lds):
    """The recorded figure; 0 above the limit, where the hosts do not ask."""
    if kernel != 'split' and lds > LDS_LIMIT:
        return 0
    return RESIDENCY[kernel][lds]


def _ceil(a, b):
    return (a + b - 1) // b


def padded_voc(V):
    return (V + 31) & ~31


def ctx_width(d, W, deep=False):
    return 2 * W if d == 1 or deep else W


def dec_lds(d, W, V, deep=False):
    """(kmax, lda, dynamic LDS bytes) of the persistent decoder: persist_dec_kmax, persist_dec_lda, persist_dec_lds_bytes."""
    Vp, C = padded_voc(V), ctx_width(d, W, deep)
    kmax = max([W] + [(Vp if n == 1 else W) + (C if n == d else 0) + W for n in range(1, d + 1)])
    return kmax, kmax + 4, 16 * (kmax + 4) * 4


def enc_lds(d, W):
    """(lda, dynamic LDS bytes) of the chain encoder: persist_enc_lda, persist_enc_lds_bytes."""
    lda = (3 * W if d >= 2 else 2 * W) + 4
    return lda, 16 * lda * 4


def decoder_form(d, W, V, B, cus=256, per_cu=None, persistent=-1, arithmetic=0, deep=False):
    """plan_persist_decode restated, and the forms persist_decode_kernel takes on that plan.  per_cu: the runtime's figure (None: the
    recorded one).  -> dict: the record of the plan (applies, reason, kmax, lda, lds, per_cu, g_lstm, g_att, g_plain, counters) and,
    where the launch applies, the named forms:
      lstm_own     most tiles of one layer a tile workgroup walks (`for (t = g; t < NT; t += g_lstm)`)
      lstm_round   'full' if every tile workgroup owns that many, else 'partial'
      plain_own    most query / logits tasks of a step a plain workgroup walks; query_idle / logits_idle: the last task of a row
                   block has waves without a column tile
      attention    'rows' (a wave keeps its row: one task per workgroup) or 'tasks'; attention_why: which of the conditions
                   ('width', 'ctx', 'rows') sent it to the task form; att_own: most row quarters a workgroup walks
      stats        greedy_tie_cases.greedy_form(V)"""
    Vp, C = padded_voc(V), ctx_width(d, W, deep)
    kmax, lda, lds = dec_lds(d, W, V, deep)
    if per_cu is None:
        per_cu = residency('decode', lds)
    if lds > LDS_LIMIT:
        per_cu = 0
    f = dict(applies=False, kmax=kmax, lda=lda, lds=lds, per_cu=per_cu, g_lstm=0, g_att=0, g_plain=0, counters=0)

    def no(reason):
        f['reason'] = reason
        return f
    if persistent == 0:
        return no('off')
    if arithmetic:
        return no('split_arithmetic')
    if cus < MIN_CUS:
        return no('cus')
    if d > MAX_DEPTH:
        return no('depth')
    if per_cu < 1:
        return no('lds')
    nrb, nug = _ceil(B, 16), W // 16
    nq4, nl4 = _ceil(W // 16, 4), _ceil(Vp // 16, 4)
    slots = cus * per_cu
    f['g_lstm'] = min(nrb * nug, slots * 4 // 8)
    f['g_plain'] = min(nrb * (nq4 + nl4), max(slots * 2 // 8, 4))
    f['g_att'] = min(nrb * 4, max(slots // 8, 4, slots - f['g_lstm'] - f['g_plain']))
    f['counters'] = (nrb * (d + 3) * 32 + 32) * 4
    if persistent == 1:
        if B > ROWS_FORCED:
            return no('not_worth')
    elif B > ROWS_DEFAULT or _ceil(nrb * nug, max(1, slots * 4 // 8)) > OWN_DEFAULT:
        return no('not_worth')
    f['applies'] = True
    f['lstm_own'] = _ceil(nrb * nug, f['g_lstm'])
    f['lstm_round'] = 'full' if (nrb * nug) % f['g_lstm'] == 0 else 'partial'
    f['plain_own'] = _ceil(nrb * (nq4 + nl4), f['g_plain'])
    f['query_idle'], f['logits_idle'] = (W // 16) % 4 != 0, (Vp // 16) % 4 != 0
    why = tuple(k for k, on in (('width', W > 256), ('ctx', C > 256), ('rows', nrb * 4 > f['g_att'])) if on)
    f['attention'], f['attention_why'] = ('tasks' if why else 'rows'), why
    f['att_own'] = _ceil(nrb * 4, f['g_att'])
    f['stats'] = greedy_form(V)
    return no('ok')


def encoder_form(d, W, B, cus=256, per_cu=None, persistent=-1, split=False, residual=False, deep=False):
    """plan_persist_encode restated.  -> dict(form 'chain' / 'split' / 'none', reason, grid, per_cu, own1, ownn, counters) and, where
    there is a form, round1 / roundn: 'full' if every workgroup owns own1 (ownn) tiles of the phase, else 'partial' ('-': the phase
    has no tile)."""
    f = dict(form='none', grid=0, per_cu=0, own1=0, ownn=0, counters=0)

    def no(reason):
        f['form'], f['reason'] = 'none', reason
        return f
    if persistent == 0:
        return no('off')
    if cus < MIN_CUS:
        return no('cus')
    if d > MAX_DEPTH:
        return no('depth')
    if (residual and d >= 3) or (deep and d >= 2):
        return no('topology')
    if per_cu is None:
        per_cu = residency('split', SPLIT_LDS) if split else residency('encode', enc_lds(d, W)[1])
    if not split and enc_lds(d, W)[1] > LDS_LIMIT:
        per_cu = 0
    f['per_cu'] = per_cu
    if per_cu < 1:
        return no('lds')
    side = 32 if split else 16
    ntile = _ceil(B, side) * (W // side)
    grid = f['grid'] = min(max(2, d - 1) * ntile, per_cu * cus)
    f['own1'], f['ownn'] = _ceil(2 * ntile, grid), _ceil((d - 1) * ntile, grid)
    f['counters'] = (_ceil(B, side) * (d + 1) * 32 + 32) * 4
    maxt = SPLIT_MAX_TILES if split else ENC_MAX_TILES
    if f['own1'] > maxt or f['ownn'] > maxt:
        return no('own')
    if persistent == 1:
        pays = B <= ROWS_FORCED
    elif split:
        pays = B <= SPLIT_DEFAULT_ROWS
    else:
        pays = B <= ROWS_DEFAULT and f['own1'] <= OWN_DEFAULT and f['ownn'] <= OWN_DEFAULT
    if not pays:
        return no('not_worth')
    f['form'], f['reason'] = ('split' if split else 'chain'), 'ok'
    f['round1'] = 'full' if (2 * ntile) % grid == 0 else 'partial'
    f['roundn'] = '-' if d == 1 else 'full' if ((d - 1) * ntile) % grid == 0 else 'partial'
    return f


# ------------------------------------------------------------------------------------------------------------------ the cases
# arith: 0 = the fp32-input chain (persistent encoder of persist.hip, greedy decodes: the persistent decoder), 2 = the split
# arithmetic (persistent encoder of persist_split.hip behind a beam search).  enc / dec: under which value of the option
# "persistent" the encoder pass / the greedy decode is ONE persistent launch on 256 CUs -- 'default' (-1 and 1), 'forced' (1 only),
# 'none' (neither; the per-step kernels run whatever the option says); dec None: the case has no greedy decode.
Case = collections.namedtuple('Case', 'name arith d W V B L enc dec modes')


def _c(name, arith, d, W, V, B, L, enc, dec, modes=(0,)):
    return Case(name, arith, d, W, V, B, L, enc, dec, tuple(modes))


CASES = [
    # depth 2, width 256: 16 unit groups, two workgroups per CU -> 256 tile workgroups, 128 plain ones, 128 for the attention rows
    _c('d2_w256_v256_b256', 0, 2, 256, 256, 256, 6, 'default', 'default'),          # configs[1]'s shape: one tile each, exactly
    _c('d2_w256_v256_b272', 0, 2, 256, 256, 272, 6, 'default', 'default'),          # a 17th row block: 16 workgroups own two tiles
    _c('d2_w256_v256_b512', 0, 2, 256, 256, 512, 6, 'default', 'default'),          # the rule's upper edge: two tiles each
    _c('d2_w256_v40_b528', 0, 2, 256, 40, 528, 6, 'forced', 'forced', (0, 1)),      # three tiles; 132 row quarters on 128 workgroups
    # width 512: 98 560 bytes of staged rows, one workgroup per CU -> 128 tile workgroups, 64 plain ones; attention by tasks (W > 256)
    _c('d2_w512_v256_b80', 0, 2, 512, 256, 80, 6, 'default', 'default', (0, 1)),
    _c('d2_w512_v256_b128', 0, 2, 512, 256, 128, 6, 'default', 'default', (0, 1)),
    # depth 1: top and first layer in one, step 0 stages [ctx | h]; C = 2W = 512: attention by tasks; the encoder has no phase B
    _c('d1_w256_v40_b40', 0, 1, 256, 40, 40, 6, 'default', 'default', (0, 1)),
    # 6 query tiles and 18 logits tiles: the last task of each has two idle waves; V > 256: statistics a row at a time
    _c('d2_w96_v257_b17', 0, 2, 96, 257, 17, 7, 'default', 'default', (0, 1)),
    # row-block edges
    _c('d2_w64_v50_b1', 0, 2, 64, 50, 1, 9, 'default', 'default', (0, 1)),
    _c('d2_w64_v50_b15', 0, 2, 64, 50, 15, 9, 'default', 'default'),
    _c('d2_w64_v50_b16', 0, 2, 64, 50, 16, 9, 'default', 'default'),
    _c('d2_w64_v50_b17', 0, 2, 64, 50, 17, 9, 'default', 'default', (0, 1)),
    # the shortest passes: T = 1 (the first step is the last: cfin from the zero-state cell) and T = 2
    _c('d2_w64_v50_b20_t1', 0, 2, 64, 50, 20, 0, 'default', 'default'),
    _c('d3_w64_v50_b20_t2', 0, 3, 64, 50, 20, 1, 'default', 'default'),
    # the encoder's phase B on three tiles (forced) beside a decoder on two (default)
    _c('d4_w256_v40_b512', 0, 4, 256, 40, 512, 5, 'forced', 'default'),
    # depth 8: 512 workgroups on 1168 + 4088 tiles: own1 3, ownn 8 = PENC_MAXT; one row block more: ownn 9, no form even when forced
    _c('d8_w128_v40_b1168', 0, 8, 128, 40, 1168, 5, 'forced', 'forced'),
    _c('d8_w128_v40_b1184', 0, 8, 128, 40, 1184, 5, 'none', None),
    # the LDS edge: 16 rows of 3 x 768 + 4 floats are 147 712 of 153 600 bytes in both kernels; width 800 has no form (153 856)
    _c('d2_w768_v40_b16', 0, 2, 768, 40, 16, 5, 'default', 'default'),
    _c('d2_w800_v40_b16', 0, 2, 800, 40, 16, 5, 'none', 'none'),
    # ---- the split arithmetic's encoder: tiles of 32 x 32, two workgroups per CU -> 512 workgroups
    _c('split_d2_w128_v64_b40', 2, 2, 128, 64, 40, 7, 'default', None),              # one tile each
    _c('split_d1_w128_v64_b33', 2, 1, 128, 64, 33, 7, 'default', None),              # no phase B; a second row block of one row
    _c('split_d2_w64_v50_b20_t1', 2, 2, 64, 50, 20, 0, 'default', None),
    # (depth 4, width 512, 256 lines would own two phase-B tiles at one workgroup per CU; the runtime admits two, so depth 8:)
    _c('split_d8_w512_v40_b160', 2, 8, 512, 40, 160, 5, 'default', None),            # 560 phase-B tiles on 512 workgroups: own 2
    _c('split_d8_w128_v40_b2336', 2, 8, 128, 40, 2336, 5, 'forced', None),           # 2044 phase-B tiles: own 4 = PS_MAXT
    _c('split_d8_w128_v40_b2368', 2, 8, 128, 40, 2368, 5, 'none', None),             # 2072: own 5, no form
]
IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
# No handle can be made at depth 9 (casv_model_create: 1..8), so the plans' depth rule is held on the CPU alone
# (tests/test_persist_form_cases.py); the device keeps it unreachable.
DEPTH_9 = dict(d=9, W=64, V=50, B=20)


def forms(case, cus=256, persistent=-1, per_cu=None):
    """(encoder form, decoder form or None) of a case; per_cu: (encoder kernel's, decoder's) figures, None = the recorded ones."""
    e_pc, d_pc = per_cu if per_cu else (None, None)
    enc = encoder_form(case.d, case.W, case.B, cus=cus, per_cu=e_pc, persistent=persistent, split=case.arith > 0)
    dec = None
    if case.dec is not None:
        dec = decoder_form(case.d, case.W, case.V, case.B, cus=cus, per_cu=d_pc, persistent=persistent, arithmetic=case.arith)
    return enc, dec


def expected(rule, persistent):
    """Whether a part marked `rule` is one persistent launch under the option value `persistent`."""
    return persistent != 0 and (rule == 'default' or (rule == 'forced' and persistent == 1))


# ---- the records both sides print (tests/persist_plan_driver.cpp)
def driver_lines(case, cus, persistent, per_cu=None):
    """The driver's input lines of a case: E name d W residual deep B cus per_cu persistent split / D name d W Vp C B cus per_cu
    persistent arithmetic."""
    split = case.arith > 0
    e_pc = per_cu[0] if per_cu else (residency('split', SPLIT_LDS) if split else residency('encode', enc_lds(case.d, case.W)[1]))
    out = ['E %s %d %d 0 0 %d %d %d %d %d' % (case.name, case.d, case.W, case.B, cus, e_pc, persistent, int(split))]
    if case.dec is not None:
        d_pc = per_cu[1] if per_cu else residency('decode', dec_lds(case.d, case.W, case.V)[2])
        out.append('D %s %d %d %d %d %d %d %d %d %d' % (case.name, case.d, case.W, padded_voc(case.V), ctx_width(case.d, case.W), case.B,
                                                        cus, d_pc, persistent, case.arith))
    return out


def encoder_record(f):
    return 'E form=%s reason=%s grid=%d per_cu=%d own1=%d ownn=%d counters=%d' % (
        f['form'], f['reason'], f['grid'], f['per_cu'], f['own1'], f['ownn'], f['counters'])


def decoder_record(f):
    return 'D applies=%d reason=%s kmax=%d lda=%d lds=%d per_cu=%d g_lstm=%d g_att=%d g_plain=%d counters=%d' % (
        f['applies'], f['reason'], f['kmax'], f['lda'], f['lds'], f['per_cu'], f['g_lstm'], f['g_att'], f['g_plain'], f['counters'])


# ------------------------------------------------------------------------------------------------------------------ the inputs
_BUILT, _ORACLES = {}, {}


def build(case):
    """decode_noise_cases.build_encoder of a case, ragged: (cfg, float32 weights, oracle input x (B, T, V), device input idx (B, T)).
    Computed once per process and left as it is."""
    if case.name not in _BUILT:
        cfg, w, x, (idx, _) = dn.build_encoder((case.name, case.d, case.W, case.V, case.B, case.L, {}, 1, case.arith, -1))
        T = idx.shape[1]
        if case.B >= 3 and T >= 2:
            idx[1, T // 2:] = -1
            x[1, T // 2:] = 0
        _BUILT[case.name] = (cfg, w, x, idx)
    return _BUILT[case.name]


def oracles(case):
    """(float32, float64) oracle encoder outputs of a case, computed once per process and left as they are."""
    if case.name not in _ORACLES:
        cfg, w, x, _ = build(case)
        _ORACLES[case.name] = (dn.oracle_encoder(cfg, w, x, np.float32), dn.oracle_encoder(cfg, w, x, np.float64))
    return _ORACLES[case.name]
