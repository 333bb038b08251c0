"""Every launch form of the decode path's persistent kernels on the device (cases and forms: tests/persist_form_cases.py).

Per case, under the option "persistent" = 0, -1 and 1:
  form first   the statistics ("encoder_persistent", "encoder_persist_per_cu" / "_grid", "decoder_persistent", "decoder_persist_per_cu"
               / "_g_lstm" / "_g_att" / "_g_plain") equal the restated plan at the device's own CU count and workgroups per CU; the
               profile class "persist" counts one launch per persistent pass and none otherwise; "decode_give_ups" stays 0.  On 256
               CUs the workgroups per CU are the recorded ones (persist_form_cases.RESIDENCY) and the forms the table's; a device
               with another CU count on which a case plans to another form skips the case, with the reason.
  bits         encoder outputs and every final state, and per greedy mode characters, probabilities, lengths, alignment rows and
               the sparse window store equal the per-step kernels' bit for bit; the split arithmetic's cases compare everything a
               small beam search returns.
  float64      the encoder outputs and final states against the float64 oracle in units of the float32 oracle's own error, by
               tests/decode_noise_cases.py and its constants.  (The decoder's steps are held to float64 transitively: the per-step
               kernels by decode_noise_cases.STEP_CASES, the persistent forms by equal bits.)
The ratios are printed per case (RATIOS lines; recorded in profiles/persist_form_ratios.txt)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

os.environ.setdefault('CASV_POISON', '1')

from tests import decode_noise_cases as dn
from tests import persist_form_cases as pf

BEAM_KEYS = ('idx', 'prob', 'score', 'len', 'align', 'rej', 'n_found', 'n_steps')
OPTIONS = (0, -1, 1)
ENC_FORM_KEYS = ('form', 'reason', 'grid', 'per_cu', 'own1', 'ownn')


def _engine(case, w):
    from cor_asv_ann_amd.engine import HipEngine
    eng = HipEngine(case.d, case.W, case.V)
    eng.set_weights(w)
    eng.set_option('arithmetic', case.arith)
    return eng


def _launches(eng, call):
    """(what `call` returns, or the error code it raised; launches of the profile class "persist" it made)"""
    from cor_asv_ann_amd._native import NativeError
    eng.profile(1)
    try:
        res = call()
    except NativeError as err:
        res = err.code
    n = eng.profile_read('persist')['launches']
    eng.profile(0)
    return res, n


def _leg(eng, case, idx, p):
    """One pass of a case under "persistent" = p: results, and what the statistics and the profile say ran."""
    eng.set_option('persistent', p)
    eng.encode(idx)
    (enc, st), n = _launches(eng, eng.encoder_outputs)
    seen = {'enc': (eng.stat('encoder_persistent'), n), 'enc_plan': (eng.stat('encoder_persist_per_cu'), eng.stat('encoder_persist_grid'))}
    out = {'enc': [enc] + list(st)}
    if case.arith:
        eng.encode(idx)                            # (a fresh encoding: the search runs its own encoder pass)
        res, n = _launches(eng, lambda: eng.decode_beam(batch_size=2, want_align=True, rejection_threshold=0.5))
        seen['beam'] = (eng.stat('encoder_persistent'), n)
        out['beam'] = [res[k] for k in BEAM_KEYS]
    elif case.dec is not None:
        for mode in case.modes:                    # (on the encoding above: the launches counted are the decode's own)
            res, n = _launches(eng, lambda: eng.decode_greedy(mode=mode, want_align=True))
            seen['dec', mode] = (eng.stat('decoder_persistent'), n)
            seen['dec_plan', mode] = tuple(eng.stat('decoder_persist_' + k) for k in ('per_cu', 'g_lstm', 'g_att', 'g_plain'))
            if not isinstance(res, int):
                res = tuple(res) + eng.alignments_sparse(case.B, res[0].shape[1])
            out['dec', mode] = res
    return out, seen


def _check_form(case, p, seen, cus):
    """The statistics of a leg against the restatement at the device's own figures -> (encoder form, decoder form)."""
    enc_pc = seen['enc_plan'][0]
    dec_pc = seen['dec_plan', case.modes[0]][0] if ('dec_plan', case.modes[0]) in seen else None
    enc, dec = pf.forms(case, cus=cus, persistent=p, per_cu=(enc_pc, dec_pc))
    on = int(enc['form'] != 'none')
    assert seen['enc'] == (on, on), (case.name, p, 'encoder pass', seen['enc'], enc)
    assert seen['enc_plan'] == (enc['per_cu'], enc['grid'] if on else 0), (case.name, p, seen['enc_plan'], enc)
    if 'beam' in seen:
        assert seen['beam'] == (on, on), (case.name, p, 'the search\'s encoder pass', seen['beam'], enc)
    if dec is not None:
        for mode in case.modes:
            assert seen['dec', mode] == (int(dec['applies']), int(dec['applies'])), (case.name, p, mode, seen['dec', mode], dec)
            assert seen['dec_plan', mode] == (dec['per_cu'], dec['g_lstm'], dec['g_att'], dec['g_plain']), (case.name, p, mode, seen['dec_plan', mode], dec)
    return enc, dec


def _same(a, b, what):
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), (what, k, int((x != y).sum()))


def _same_greedy(case, mode, a, b):
    assert mode == 1 or not (isinstance(a, int) or isinstance(b, int)), (case.name, 'mode 0 has no rule to raise by', a, b)
    if isinstance(a, int) or isinstance(b, int):          # (mode 1 may raise on an all-NaN row: on both paths alike)
        assert a == b, (case.name, mode, a if isinstance(a, int) else 'ok', b if isinstance(b, int) else 'ok')
        return
    for k, name in enumerate(('idx', 'prob', 'len', 'align', 'window_lo', 'window_w')):
        x, y = a[k], b[k]
        if mode == 1 and name != 'len':                    # rows keep stepping after their line has ended; only the reported part counts
            for j in range(case.B):
                n = int(a[2][j])
                assert np.array_equal(x[j, :n], y[j, :n], equal_nan=True), (case.name, mode, name, j)
        else:
            assert np.array_equal(x, y, equal_nan=True), (case.name, mode, name)


def _quantities(case, enc_list):
    q = {'enc_out': enc_list[0]}
    for n in range(case.d):
        q['h%d' % (n + 1)], q['c%d' % (n + 1)] = enc_list[1 + 2 * n], enc_list[2 + 2 * n]
    return q


@pytest.mark.parametrize('name', pf.IDS)
def test_form_then_bits_then_float64(name):
    case = pf.BY_NAME[name]
    cfg, w, x, idx = pf.build(case)
    eng = _engine(case, w)
    try:
        cus = eng.stat('cus')
        legs = {p: _leg(eng, case, idx, p) for p in OPTIONS}
        give_ups = eng.stat('decode_give_ups')
    finally:
        eng.close()
    # ---- form first
    assert give_ups == 0, (name, 'a persistent launch gave up on this device')
    for p in OPTIONS:
        enc, dec = _check_form(case, p, legs[p][1], cus)
        # 256 CUs, the recorded workgroups per CU (under 0 the hosts do not ask the runtime: the plans carry 0)
        want_enc, want_dec = pf.forms(case, persistent=p, per_cu=(0, 0) if p == 0 else None)
        same = all(enc[k] == want_enc[k] for k in ENC_FORM_KEYS) and dec == want_dec
        print('FORM %s persistent=%d cus=%d encoder %s decoder %s' % (name, p, cus, {k: enc[k] for k in ENC_FORM_KEYS}, dec))
        if not same and cus != 256:
            pytest.skip('this device has %d CUs, not 256: %s plans to %r / %r under persistent = %d, the case is meant for %r / %r'
                        % (cus, name, enc, dec, p, want_enc, want_dec))
        assert same, (name, p, 'the runtime admits other workgroups per CU than recorded', enc, want_enc, dec, want_dec)
        assert (enc['form'] != 'none') == pf.expected(case.enc, p), (name, p)
        assert dec is None or dec['applies'] == pf.expected(case.dec, p), (name, p)
    # ---- bit for bit against the per-step kernels
    step = legs[0][0]
    for p in (-1, 1):
        out = legs[p][0]
        _same(step['enc'], out['enc'], (name, p, 'encoder outputs and final states'))
        if 'beam' in step:
            _same(step['beam'], out['beam'], (name, p, 'beam search'))
        for mode in case.modes if case.dec is not None and not case.arith else ():
            _same_greedy(case, mode, step['dec', mode], out['dec', mode])
    # ---- float64
    o32, o64 = pf.oracles(case)
    r = {p: dn.ratios(_quantities(case, legs[p][0]['enc']), o32, o64) for p in (0, 1)}
    worst = max(r[1], key=lambda k: max(r[1][k][0] / dn.C_RMS, r[1][k][1] / dn.C_MAX))
    print('RATIOS %s encoder %s: excess %.3f (worst %s: rms %.3f max %.3f); per step: excess %.3f'
          % (name, legs[1][1]['enc'][0] and ('split' if case.arith else 'chain') or 'per-step', dn.excess(r[1]), worst, r[1][worst][0], r[1][worst][1],
             dn.excess(r[0])))
    assert dn.excess(r[1]) < 1.0, (name, r[1])
    assert dn.excess(r[0]) < 1.0, (name, 'per step', r[0])


def test_no_handle_at_depth_9():
    """The plans' depth rule (no persistent form above depth 8) cannot be reached through the C ABI: no handle exists at depth 9."""
    from cor_asv_ann_amd._native import NativeError
    from cor_asv_ann_amd.engine import HipEngine
    d9 = pf.DEPTH_9
    with pytest.raises(NativeError):
        HipEngine(d9['d'], d9['W'], d9['V'])
