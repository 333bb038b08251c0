"""The training state's Keras view (csrc/keras_table.h, train_state.hip): what is set is what is read, for the weights, the
gradients and Adam's moments alike; the accessors' errors; and that a closed handle gives its device memory back."""
import gc

import numpy as np
import pytest
import torch            # (before the library loads: one HIP runtime in the process, so that torch.cuda.mem_get_info sees the device)

pytestmark = pytest.mark.gpu

from tests import train_state_cases as tc
from tests import update_cases as uc

ERR_ARG, ERR_STATE = -1, -2


def _engine(depth, flags, width=tc.W, voc=tc.V):
    from cor_asv_ann_amd.engine import HipEngine
    eng = HipEngine(depth, width, voc, **flags)
    w = tc.weights_of(depth, width, voc, flags)
    eng.set_weights(w)
    return eng, w


def _get_state(eng, name, which):
    from cor_asv_ann_amd import _native as nv
    a = np.empty(eng.pshapes[name], np.float32)
    nv.check(eng.lib.casv_train_get_state(eng.handle, name.encode(), which, nv.ptr(a), a.size))
    return a


def _set_state(eng, name, which, a):
    from cor_asv_ann_amd import _native as nv
    a = nv.carray(a, np.float32)
    nv.check(eng.lib.casv_train_set_state(eng.handle, name.encode(), which, nv.ptr(a), a.size))


@pytest.mark.parametrize('name,depth,flags', tc.CONFIGS, ids=tc.IDS)
def test_what_is_set_is_what_is_read(name, depth, flags):
    """Pack then unpack is the identity on the device path: train_weights() right behind train_begin returns the weights that were
    set, bit for bit; an all-distinct tensor set as Adam's m or v of one name comes back exactly and changes no other name's state
    (a table entry that wrote another entry's parts would); K, then R, then b of one layer leave all three as set."""
    eng, w = _engine(depth, flags)
    try:
        eng.train_begin()
        got = eng.train_weights()
        assert set(got) == set(w)
        for k in w:
            assert np.array_equal(got[k].view(np.uint32).ravel(), w[k].view(np.uint32).ravel()), k
        names = list(eng.pshapes)
        kept = {}
        for which in (0, 1):
            held = {k: _get_state(eng, k, which) for k in names}
            assert all(not a.any() for a in held.values())          # a fresh session: zeros
            start = 1.0 + 100000.0 * which
            for k in names:
                held[k] = tc.distinct(eng.pshapes[k], start)
                start += held[k].size
                _set_state(eng, k, which, held[k])
                for other in names:
                    assert np.array_equal(_get_state(eng, other, which), held[other]), (which, k, other)
            kept[which] = held
        for which in (0, 1):                                        # m and v do not share a buffer
            for k in names:
                assert np.array_equal(_get_state(eng, k, which), kept[which][k]), (which, k)
        layer = 'dec%d' % depth
        trio = {s: tc.distinct(eng.pshapes[layer + s], 5000.0 * (i + 1)) for i, s in enumerate(('_K', '_R', '_b'))}
        for s in ('_K', '_R', '_b'):
            _set_state(eng, layer + s, 0, trio[s])
        for s in ('_K', '_R', '_b'):
            assert np.array_equal(_get_state(eng, layer + s, 0), trio[s]), s
        eng.train_end()
    finally:
        eng.close()


@pytest.mark.parametrize('name,depth,flags', tc.CONFIGS, ids=tc.IDS)
def test_first_moment_is_the_gradient_accessors_gradient(name, depth, flags):
    """One deterministic mode-1 step that does not clip, from zero moments: every name's m is (1 - beta1) * g of train_gradients(),
    element by element -- the gradient accessor and the state accessor read the same layout.  Comparator and bound are
    tests/update_cases.py's (restate: m' within gamma(2) (|b1 m| + |(1 - b1) g|) + 2^-120 of the float64 product, tighter than the
    relative 2^-20 a permuted or transposed element of a random gradient misses by order 1)."""
    eng, _ = _engine(depth, flags)
    try:
        eng.set_option('deterministic', 1)
        batch = tc.batch_of(tc.V, tc.B, tc.T, tc.U)
        eng.train_begin()
        _, norm = eng.train_step(*batch, mode=2)
        eng.train_end()
        hyper = dict(uc.DEFAULT, clipnorm=float(2.0 * norm + 1.0))         # above the step's norm: nothing clips
        eng.train_begin(**hyper)
        _, norm = eng.train_step(*batch, mode=1)
        assert not uc.scale_of(hyper, norm)[1]
        g = eng.train_gradients()
        m, v, step = eng.train_state()
        assert step == 1 and set(m) == set(g) == set(eng.shapes)
        worst = 0.0
        for k in g:
            assert np.abs(g[k]).max() > 0, k
            zero = np.zeros_like(g[k])
            (m_ref, m_bound), _, _ = uc.restate(zero, zero, zero, g[k], norm, 0, hyper, m[k], v[k])
            err = float((np.abs(np.asarray(m[k], np.float64) - m_ref) / m_bound).max())
            worst = max(worst, err)
            assert err <= 1.0, (k, err)
        print('m against (1 - beta1) g, worst error in units of the bound:', worst)
        eng.train_end()
    finally:
        eng.close()


def _raises(code, text, fn, *args):
    from cor_asv_ann_amd import _native as nv
    rc = fn(*args)
    assert rc == code, (rc, code)
    msg = nv.load().casv_last_error().decode()
    assert msg == text, (msg, text)


def test_accessor_errors_keep_code_and_text():
    """The accessors' refusals: an unknown name, a capacity one short, a count one off, a frozen tensor, which = 2, no session."""
    from cor_asv_ann_amd import _native as nv
    eng, _ = _engine(2, {})
    try:
        lib, h = eng.lib, eng.handle
        n = int(np.prod(eng.pshapes['enc1_fw_K']))
        a = np.zeros(n + 1, np.float32)
        step = nv.c_int64()
        for fn, args in ((lib.casv_train_get_gradient, (h, b'E', nv.ptr(a), a.size)), (lib.casv_train_get_state, (h, b'E', 0, nv.ptr(a), a.size)),
                         (lib.casv_train_set_state, (h, b'E', 0, nv.ptr(a), a.size)), (lib.casv_train_get_step, (h, nv.ctypes.byref(step))),
                         (lib.casv_train_set_step, (h, 3)), (lib.casv_train_sync_weights, (h,)), (lib.casv_train_end, (h,))):
            _raises(ERR_STATE, 'no training session', fn, *args)
        eng.train_begin(frozen=('enc1_',))
        for fn, args in ((lib.casv_train_get_gradient, (h, b'nope', nv.ptr(a), a.size)), (lib.casv_train_get_state, (h, b'nope', 0, nv.ptr(a), a.size)),
                         (lib.casv_train_set_state, (h, b'nope', 0, nv.ptr(a), a.size)),
                         (lib.casv_train_get_state, (h, b'enc1_fw', 0, nv.ptr(a), a.size)), (lib.casv_train_get_state, (h, b'dec2_Wx', 0, nv.ptr(a), a.size))):
            _raises(ERR_ARG, "unknown tensor '%s'" % args[1].decode(), fn, *args)
        for name in (b'dec1_K', b'dec2_R', b'dec1_b', b'att_U', b'att_Wa', b'E'):
            size = int(np.prod(eng.pshapes[name.decode()]))
            _raises(ERR_ARG, 'buffer too small', lib.casv_train_get_gradient, h, name, nv.ptr(a), size - 1)
            _raises(ERR_ARG, 'buffer too small', lib.casv_train_get_state, h, name, 1, nv.ptr(a), size - 1)
            for count in (size - 1, size + 1):
                _raises(ERR_ARG, "tensor '%s' has %d values, got %d" % (name.decode(), size, count), lib.casv_train_set_state, h, name, 1, nv.ptr(a), count)
        for name in (b'enc1_fw_K', b'enc1_bw_b'):
            text = "tensor '%s' is frozen: it has no optimizer state" % name.decode()
            _raises(ERR_STATE, text, lib.casv_train_get_state, h, name, 0, nv.ptr(a), a.size)
            _raises(ERR_STATE, text, lib.casv_train_set_state, h, name, 0, nv.ptr(a), n)
        assert lib.casv_train_get_gradient(h, b'enc1_fw_K', nv.ptr(a), a.size) == 0        # (a frozen tensor has a gradient buffer)
        for fn in (lib.casv_train_get_state, lib.casv_train_set_state):
            for which in (2, -1):
                _raises(ERR_ARG, 'which must be 0 (Adam m) or 1 (Adam v)', fn, h, b'E', which, nv.ptr(a), a.size)
            _raises(ERR_ARG, 'which must be 0 (Adam m) or 1 (Adam v)', fn, h, b'nope', 2, nv.ptr(a), a.size)     # (which before the name)
            _raises(ERR_ARG, "unknown tensor 'nope'", fn, h, b'nope', 1, None, a.size)                          # (the name before the pointer)
            _raises(ERR_STATE, "tensor 'enc1_fw_R' is frozen: it has no optimizer state", fn, h, b'enc1_fw_R', 1, None, 0)
            _raises(ERR_ARG, 'null argument', fn, h, b'E', 1, None, a.size)
        _raises(ERR_ARG, 'step must be >= 0', lib.casv_train_set_step, h, -1)
        eng.train_end()
    finally:
        eng.close()


# The ownership check's model: the session's tensors alone (weights, gradients, two moments) are 4 x 12.6 M floats = 200 MiB
OWN_DEPTH, OWN_W, OWN_V, OWN_B, OWN_L = 2, 512, 40, 8, 16
PARENT_GROWTH_MIB = 16.0            # measured on the build with the hand-written release lists (docstring below)
GROWTH_SLACK_MIB = 2.0


def test_closed_handles_give_their_memory_back():
    """Coarse ownership: create, set weights, train_begin, one step, train_end, a scoring call outside a session, close -- once to warm
    up, then four more times; the device's free memory after the last cycle against after the first.  The session's tensors take
    more than 64 MiB (asserted around the first train_begin), so a state that was not released shows whatever the allocator's
    granule.  Bound: the growth the build before the buffers owned their memory showed on the same cycles, plus 2 MiB (one granule).
    Measured over the four cycles (train_begin taking 252 / 250 MiB): 16.00 MiB with the hand-written release lists, 16.00 MiB with
    the owning buffers -- the same 16 MiB either way, none of it the 250 MiB a state that stayed behind would add per cycle."""
    from cor_asv_ann_amd.engine import HipEngine
    w = tc.weights_of(OWN_DEPTH, OWN_W, OWN_V, {})
    batch = tc.batch_of(OWN_V, OWN_B, OWN_L, OWN_L)
    free = lambda: torch.cuda.mem_get_info()[0] / 2.0 ** 20
    begin_took = []

    def cycle():
        eng = HipEngine(OWN_DEPTH, OWN_W, OWN_V)
        try:
            eng.set_weights(w)
            before = free()
            eng.train_begin()
            begin_took.append(before - free())
            eng.train_step(*batch, mode=1)
            eng.train_end()
            eng.score_targets(*batch[:4])
        finally:
            eng.close()
        gc.collect()
        torch.cuda.synchronize()
    cycle()
    warm = free()
    for _ in range(4):
        cycle()
    growth = warm - free()
    print('train_begin took %.1f MiB; growth over four cycles %.2f MiB' % (begin_took[0], growth))
    assert begin_took[0] >= 64.0
    assert growth <= PARENT_GROWTH_MIB + GROWTH_SLACK_MIB
