"""What the five train-step entries refuse in common (train.hip, check_step_args / run_step), called on the library directly: a
null enc_idx, B = 0 and mode 3 are CASV_ERR_ARG, a valid call without casv_train_begin is CASV_ERR_STATE; a refusal leaves the
session's step count, weights and moments bit for bit as they were, and a valid step afterwards succeeds."""
from ctypes import byref, c_double

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEPTH, WIDTH, V, B, T, U, K, N = 1, 32, 37, 2, 5, 4, 3, 2
CASV_ERR_ARG, CASV_ERR_STATE = -1, -2
ENTRIES = ('hard', 'soft', 'risk', 'sampled', 'sampled_cut')


def _batch():
    rng = np.random.default_rng(5)
    a = {'enc_idx': rng.integers(0, V, (B, T, 1)).astype(np.int32), 'dec_in': rng.integers(0, V, (B, U)).astype(np.int32),
         'dec_out': rng.integers(0, V, (B, U)).astype(np.int32), 'weights': np.ones((B, U), np.float32),
         'soft_idx': np.stack([rng.permutation(V)[:K] for _ in range(B * U)]).reshape(B, U, K).astype(np.int32),
         'soft_q': rng.random((B, U, K)).astype(np.float32), 'cost': np.array([0.25, 0.75], np.float32),
         'mixes': np.empty((2, B, U), np.int32)}
    return a


def _call(eng, entry, a, mode=1, batch=B, enc_idx=True):
    """The entry's return code on the batch `a`, with the arguments the bad calls change."""
    import cor_asv_ann_amd._native as nv
    lib, p = eng.lib, nv.ptr
    loss, norm = c_double(), c_double()
    head = (eng.handle, mode, batch, T, U, 1, p(a['enc_idx']) if enc_idx else None, None, p(a['dec_in']))
    hard = head + (p(a['dec_out']), p(a['weights']), None, None, None)
    sched = nv.SchedParams(3, 1, 0.5, 1.0, 1, 2)        # ratio 0.5, the sampled pick, 2 passes
    if entry == 'hard':
        return lib.casv_train_step(*hard, byref(loss), byref(norm))
    if entry == 'soft':
        return lib.casv_train_step_soft(*head, K, p(a['soft_idx']), p(a['soft_q']), p(a['weights']), None, None, None, byref(loss), byref(norm))
    if entry == 'risk':
        return lib.casv_train_step_risk(*hard, N, p(a['cost']), 1.0, None, None, byref(loss), byref(norm))
    if entry == 'sampled':
        return lib.casv_train_step_sampled(*hard, byref(sched), p(a['mixes']), byref(loss), byref(norm))
    cut = nv.SampleCut(5, 0.9)
    return lib.casv_train_step_sampled_cut(*hard, byref(sched), byref(cut), p(a['mixes']), byref(loss), byref(norm))


def _state(eng):
    m, v, step = eng.train_state()
    return step, eng.train_weights(), m, v


@pytest.mark.parametrize('entry', ENTRIES)
def test_common_refusals_leave_the_session_untouched(entry):
    from cor_asv_ann_amd.engine import HipEngine
    from cor_asv_ann_amd.synthetic import ModelConfig, make_weights
    eng = HipEngine(DEPTH, WIDTH, V)
    try:
        eng.set_weights(make_weights(ModelConfig(depth=DEPTH, width=WIDTH, voc_size=V)))
        a = _batch()
        assert _call(eng, entry, a) == CASV_ERR_STATE           # no session yet
        eng.train_begin()
        assert _call(eng, entry, a) == 0
        before = _state(eng)
        assert before[0] == 1
        for what, change, code in (('null enc_idx', dict(enc_idx=False), CASV_ERR_ARG), ('B = 0', dict(batch=0), CASV_ERR_ARG),
                                   ('mode 3', dict(mode=3), CASV_ERR_ARG)):
            assert _call(eng, entry, a, **change) == code, what
            after = _state(eng)
            assert after[0] == before[0], what
            for x, y in zip(after[1:], before[1:]):
                assert set(x) == set(y)
                for k in x:
                    assert x[k].tobytes() == y[k].tobytes(), (what, k)
        assert _call(eng, entry, a) == 0                        # (the session still works)
        assert eng.train_state()[2] == 2
        eng.train_end()
    finally:
        eng.close()
