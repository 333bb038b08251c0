"""The device-packed result records on a real MI355X, at their edges (tests/record_cases.py): pack_records_kernel behind
casv_records_reset / _append / _read / _device_ptr and casv_comm_all_gather_records, for every case of the table against
`expected_records` on the arrays the SAME decode call returned -- the kernel's inputs are the device's arrays, so the reference is
computed from those, not from the oracle.

Exact: characters, probability bit patterns, length, flag and (beam) score words.  The greedy score: within (len + 4) * 2**-52
relative of the float64 restatement (a double log of at most 1 ulp, a sum of non-negative terms in double, one division).  The
device's own first end-of-line steps and `len == 0` rows must be the planned ones: a device that leaves the table fails, it does
not pass on a smaller table.  tests/test_record_cases.py shows on the CPU that the plan is the oracle's, with a logit gap that makes
the device follow it, and that each mistake `expected_records` can be switched to changes a record of the table."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

os.environ.setdefault('CASV_POISON', '1')      # read once by the library, at its first allocation

from cor_asv_ann_amd import sharding
from tests.record_cases import (BY_NAME, C_I, CH_A, CH_SPARE, CH_X, CH_Y, EOS, HOST_SCORE_BOUND, I_C, V, VARIANTS, WIDTH, UNMAPPED,
                                counting_weights, expected_records, first_eos, sparse_lines, xs)

ERR_ARG, ERR_STATE = -1, -2


def _engine(beta, **options):
    from cor_asv_ann_amd.engine import HipEngine
    eng = HipEngine(1, WIDTH, V)
    eng.set_weights(counting_weights(beta))
    eng.set_option('eos', EOS)
    for k, v in options.items():
        eng.set_option(k, v)
    return eng


def _decode(eng, case, steps=None):
    """encode + the case's decode call -> (the arrays it returned, S)."""
    eng.encode(case.idx, case.val)
    if case.kind == 'greedy':
        gi, gp, _, _ = eng.decode_greedy(mode=0, steps=steps)
        return dict(idx=gi, prob=gp), gi.shape[1]
    res = eng.decode_beam(steps=steps, **case.beam_kwargs())
    return res, res['idx'].shape[1]


def _same_records(got, want, greedy, what):
    """Every word equal; the greedy score within (len + 4) * 2**-52 relative."""
    S = (want.shape[1] - 4) // 2
    words = np.ones(want.shape[1], bool)
    if greedy:
        words[2 * S + 1:2 * S + 3] = False
    bad = np.argwhere(got[:, words] != want[:, words])
    assert not len(bad), (what, bad[:8].tolist())
    if greedy:
        a, b = sharding.unpack_records(got)[3], sharding.unpack_records(want)[3]
        n = want[:, 2 * S]
        err = np.abs(a - b) / np.where(b != 0, np.abs(b), 1.0)
        print('%s: greedy score, largest relative difference from the restatement %.2f * 2**-52 (bound (len + 4) * 2**-52)'
              % (what, float(err.max()) * 2.0 ** 52))
        assert (err <= (n + 4) * 2.0 ** -52).all(), (what, (err * 2.0 ** 52).tolist())
        assert np.array_equal(a[b == 0], b[b == 0])


def _planned(case, out, S, what):
    """The device's own arrays are inside the table."""
    if case.kind == 'greedy':
        got = first_eos(out['idx'], EOS)
        for j, want in enumerate(case.planned_eos(S)):
            assert want is None or got[j] == want, (what, j, int(got[j]), want)
    else:
        assert [bool(n) for n in out['len'][::case.max_results]] == case.found, (what, out['len'].tolist())
        assert [bool(n) for n in out['n_found']] == case.found, (what, out['n_found'].tolist())
        if case.max_results > 1:
            assert (out['len'] > 0).all(), what


FORMS = [(name, steps, form) for name, steps in VARIANTS for form in ((1, 0) if BY_NAME[name].kind == 'greedy' else (0, 2))]


@pytest.mark.parametrize('name,steps,form', FORMS)
def test_the_records_of_a_case(name, steps, form):
    """form: `persistent` 1 / 0 for the greedy cases, `arithmetic` 0 / 2 for the beam."""
    case = BY_NAME[name]
    eng = _engine(case.beta, **({'persistent': form} if case.kind == 'greedy' else {'arithmetic': form}))
    try:
        out, S = _decode(eng, case, steps)
        assert S == case.S(steps)
        eng.records_reset(case.B + 2, S)
        eng.records_append(1)
        got = eng.records_read()
    finally:
        eng.close()
    what = (name, steps, form)
    _planned(case, out, S, what)
    assert got.shape == (case.B + 2, 2 * S + 4)
    assert not got[0].any() and not got[-1].any(), what                 # rows nobody wrote: found = 0
    _same_records(got[1:-1], expected_records(case.idx, case.val, out, EOS, S), case.kind == 'greedy', what)


def test_placement_of_several_appends_in_one_buffer():
    """One buffer of 40 rows: greedy_short at 0, greedy_chunks at 7, greedy_short again at 30, all with S = 260.  Every appended range
    is its expectation, every other row all zero; casv_records_device_ptr reports the buffer's bytes; with one rank,
    casv_comm_all_gather_records returns what casv_records_read does."""
    short, chunks = BY_NAME['greedy_short'], BY_NAME['greedy_chunks']
    S, rows = chunks.S(), 40
    eng = _engine(short.beta)
    try:
        eng.records_reset(rows, S)
        want = np.zeros((rows, 2 * S + 4), np.int32)
        for case, at in ((short, 0), (chunks, 7), (short, 30)):
            out, s = _decode(eng, case, S)
            assert s == S
            _planned(case, out, S, (case.name, at))
            eng.records_append(at)
            want[at:at + case.B] = expected_records(case.idx, case.val, out, EOS, S)
        got = eng.records_read()
        ptr, nbytes = eng.records_device_ptr()
        comm = sharding.NativeComm(eng, rank=0, world=1)
        try:
            gathered = comm.all_gather_device_records(rows)
        finally:
            comm.close()
    finally:
        eng.close()
    assert ptr and nbytes == rows * (2 * S + 4) * 4
    written = np.zeros(rows, bool)
    for case, at in ((short, 0), (chunks, 7), (short, 30)):
        written[at:at + case.B] = True
        _same_records(got[at:at + case.B], want[at:at + case.B], True, (case.name, at))
    assert not got[~written].any()
    assert np.array_equal(gathered, got)


def _refused(eng, offset, code, before):
    from cor_asv_ann_amd._native import NativeError
    with pytest.raises(NativeError) as err:
        eng.records_append(offset)
    assert err.value.code == code, str(err.value)
    assert len(str(err.value).split(': ', 1)[1]) > 10, str(err.value)          # a message
    assert np.array_equal(eng.records_read(), before)                           # the buffer as it was
    return str(err.value)


def test_append_refuses_what_it_cannot_pack_and_leaves_the_buffer_alone():
    case, longer = BY_NAME['greedy_short'], BY_NAME['greedy_confmat']
    eng = _engine(case.beta)
    try:
        out, S = _decode(eng, case)
        eng.records_reset(5, S)
        eng.records_append(1)
        before = eng.records_read()
        assert before[1:4, -1].all() and not before[0].any() and not before[4].any()
        # S different from the buffer's
        _decode(eng, case, S - 2)
        _refused(eng, 1, ERR_ARG, before)
        # row_offset + B beyond the buffer, and a negative offset
        _decode(eng, case)
        _refused(eng, 3, ERR_ARG, before)
        _refused(eng, -1, ERR_ARG, before)
        eng.records_append(2)                                   # (the same call inside the buffer is taken)
        before = eng.records_read()
        assert before[2:5, -1].all()
        # before any decode call of the encoded batch
        eng.encode(case.idx, case.val)
        _refused(eng, 0, ERR_STATE, before)
        # after a per-line greedy decode (mode 1)
        eng.decode_greedy(mode=1, steps=S)
        _refused(eng, 0, ERR_STATE, before)
        # after the decode's buffers were released: a later batch took them (a larger one: reallocated), or a single decoder step
        _decode(eng, case)
        eng.encode(longer.idx, longer.val)
        _refused(eng, 0, ERR_STATE, before)
        _decode(eng, case)
        _, states = eng.encoder_outputs()
        eng.decoder_step(np.arange(case.B, dtype=np.int32), np.zeros((case.B, V), np.float32), states, np.zeros((case.B, case.T), np.float32))
        _refused(eng, 0, ERR_STATE, before)
    finally:
        eng.close()
    # without a buffer
    eng = _engine(case.beta)
    try:
        _decode(eng, case)
        from cor_asv_ann_amd._native import NativeError
        with pytest.raises(NativeError) as err:
            eng.records_append(0)
        assert err.value.code == ERR_STATE
    finally:
        eng.close()


def stale_batches():
    """(first batch: 6 lines x 20 positions, its first line all padding; second batch: 4 lines x 10 positions) -- the second is
    no larger than the first in B * T and in B, so that a kernel reading the first batch's inputs with the second's shape reads
    stale but allocated memory."""
    first = sparse_lines([''] + [xs(19)] * 5)
    second = sparse_lines([xs(9), xs(1), xs(3), xs(5)])
    assert first[0].shape == (6, 20, 1) and second[0].shape == (4, 10, 1)
    return first, second


def test_append_refuses_lines_that_casv_encode_has_not_seen():
    """casv_set_encoder_outputs installs encoder outputs computed elsewhere and leaves the input lines of the last casv_encode on
    the device.  The records need the input lines (padding decisions, the beam's fallback): casv_records_append must refuse.
    Without the guard the kernel read the earlier batch's lines with the new batch's B and T: here the first line of the earlier
    batch is padding, its 20 empty slots were read as lines 0 and 1 of the new batch -- two all-zero records for lines that
    were decoded."""
    (idx1, val1), (idx2, val2) = stale_batches()
    eng = _engine(3.0)
    try:
        eng.encode(idx2, val2)
        enc, states = eng.encoder_outputs()
        eng.encode(idx1, val1)
        eng.decode_greedy(mode=0)
        eng.set_encoder_outputs(enc, states)
        gi, gp, _, _ = eng.decode_greedy(mode=0)
        assert list(first_eos(gi, EOS)) == [9, 1, 3, 5]                # (the decode itself is the second batch's)
        S = gi.shape[1]
        eng.records_reset(4, S)
        before = eng.records_read()
        assert not before.any()
        message = _refused(eng, 0, ERR_STATE, before)
        assert 'casv_encode' in message
        # the same lines through casv_encode are taken
        eng.encode(idx2, val2)
        gi, gp, _, _ = eng.decode_greedy(mode=0)
        eng.records_append(0)
        _same_records(eng.records_read(), expected_records(idx2, val2, dict(idx=gi, prob=gp), EOS, S), True, 'encoded')
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------- the facade
def _facade(beta, **kw):
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence
    s2s = Sequence2Sequence()
    s2s.depth, s2s.width = 1, WIDTH
    s2s.mapping, s2s.voc_size = (C_I, I_C), V
    for k, v in kw.items():
        setattr(s2s, k, v)
    s2s.configure(); s2s.set_weights(counting_weights(beta)); s2s.status = 2
    return s2s


_Y12 = CH_Y * 12
FAST_BATCHES = [[xs(65), xs(0), xs(63), ''], [xs(64), xs(65), xs(2)], [xs(65), xs(31), xs(1), xs(62)]]
BEAM_BATCHES = [[xs(2, _Y12), xs(6), _Y12 + UNMAPPED + CH_X + '\n', xs(3, _Y12)], [xs(15), xs(3), xs(2, _Y12)], [xs(3, _Y12), xs(10), xs(15)]]


def _confidences(batches, zero):
    """All 1.0, except line `zero[1]` of batch `zero[0]`: 0.0 at its positions `zero[2]`."""
    conf = [[[1.0] * len(t) for t in lines] for lines in batches]
    for t in zero[2]:
        conf[zero[0]][zero[1]][t] = 0.0
    return conf


@pytest.mark.parametrize('mode,with_conf', [('fast', False), ('fast', True), ('beam', False), ('beam', True)])
def test_records_appended_through_correct_batches(mode, with_conf):
    """`correct_batches(..., after_decode=...)` over three batches of the table's lines (each batch of one padded length, so that
    all share one S): the records appended on the device equal sharding.records_from_lines of what correct_batches yielded, word for
    word -- but the greedy score, which the host path computes from float32 logarithms: within HOST_SCORE_BOUND relative
    (tests/record_cases.py)."""
    fast = mode == 'fast'
    batches = FAST_BATCHES if fast else BEAM_BATCHES
    T = max(len(t) for lines in batches for t in lines)
    assert all(max(map(len, lines)) == T for lines in batches)
    S = 2 * T
    # fast: a line with confidence 0 everywhere is a padding line; beam: two zero confidences inside a line that falls back
    conf = _confidences(batches, (2, 1, range(32)) if fast else (0, 3, (12, 14))) if with_conf else None
    s2s = _facade(3.0) if fast else _facade(8.0, batch_size=4, rejection_threshold=0.0)
    offsets = np.cumsum([0] + [len(lines) for lines in batches])
    eng = s2s._require_engine()
    eng.records_reset(int(offsets[-1]), S)
    stream = [(lines, conf[k]) for k, lines in enumerate(batches)] if with_conf else batches
    lines, probs, scores = [], [], []
    for res in s2s.correct_batches(stream, fast=fast, greedy=fast, alignments=False, after_decode=lambda k: eng.records_append(int(offsets[k]))):
        lines += res[0]; probs += res[1]; scores += res[2]
    got = eng.records_read()
    host = sharding.records_from_lines(lines, probs, scores, s2s._codepoint_lut(), S)
    length = sharding.unpack_records(got)[2]
    if fast:
        want = [66, 1, 64, 0, 65, 66, 3, 66, 32, 2, 63]
        if with_conf:
            want[8] = 0
        assert list(length) == want
    else:
        assert list(length) == [15, 7, 15, 16, 16, 4, 15, 16, 11, 16]
        fallen_back = [0, 2, 3, 6, 7]                   # the lines with twelve `y`: their input, score 0
        assert [j for j, s in enumerate(scores) if float(s) == 0] == fallen_back
    words = np.ones(2 * S + 4, bool)
    if fast:
        words[2 * S + 1:2 * S + 3] = False
        a, b = sharding.unpack_records(host)[3], sharding.unpack_records(got)[3]
        err = np.abs(a - b) / np.where(b != 0, np.abs(b), 1.0)
        print('greedy score, host path against the device record: largest relative difference %.3e (bound %.3e)' % (err.max(), HOST_SCORE_BOUND))
        assert (err <= HOST_SCORE_BOUND).all(), err.tolist()
    bad = np.argwhere(got[:, words] != host[:, words])
    assert not len(bad), bad[:8].tolist()


def test_the_fallback_of_a_confusion_network_line():
    """A confusion-network line without a finished hypothesis.  The device follows its per-position rule: of the alternatives at
    a position the one with the highest confidence, the lowest slot among equals, index 0 where there is none (the case
    beam_unfound_confmat of the table holds it to `expected_records`).  The host string follows the reference
    (seq2seq.py:826-836): `chunk[0][0]`, the first alternative's whole string per chunk, nothing for an empty chunk.  The two differ
    where the first alternative has several characters (the device then takes, at the later positions, the best among the
    alternatives that reach that far) and at an empty chunk (no position on the device, none in the string either -- but a chunk
    whose first alternative is shorter than another one leaves positions the host string does not have); bench.py therefore packs
    such workloads on the host.  For single-character alternatives, best first, and no empty chunk both agree: asserted here."""
    line = [[(CH_Y, 1.0)]] * 12 + [[(CH_X, 0.6), (CH_A, 0.4)], [(CH_SPARE, 0.7), (CH_X, 0.2), (CH_A, 0.1)], [(UNMAPPED, 0.5), (CH_A, 0.3)],
                                   [('\n', 1.0)]]
    s2s = _facade(8.0, batch_size=4, rejection_threshold=0.0)
    lines, probs, scores, _ = s2s.correct_lines([line], conf=[line], fast=False, greedy=False, alignments=False)
    assert lines == [CH_Y * 12 + CH_X + CH_SPARE + UNMAPPED + '\n'] and scores == [0]
    eng = s2s.engine
    S = 2 * len(line)
    eng.records_reset(1, S)
    eng.records_append(0)
    got = eng.records_read()
    host = sharding.records_from_lines(lines, probs, scores, s2s._codepoint_lut(), S)
    assert np.array_equal(got, host), np.argwhere(got != host).tolist()
    assert list(got[0, :16]) == [C_I[CH_Y]] * 12 + [C_I[CH_X], C_I[CH_SPARE], 0, EOS]
