"""The activation functions every kernel inlines (csrc/common.h: fast_tanh, fast_sigmoid, lstm_cell) against float64, through the
test-support entry casv_debug_activation: absolute error on a dense sweep of float32 inputs, the Taylor branch's switch at |x| = 0.25,
the saturation ranges, sigmoid's subnormal results, special values, tanh's odd symmetry bit for bit, and the LSTM cell."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# Largest absolute error against float64 over every input below: measured on an MI355X 1.05e-7 (tanh) and 1.06e-7 (sigmoid)
# (profiles/r09_activation_error.txt); committed at about 2x that.
ACT_BOUND = 2.0e-7


@pytest.fixture(scope='module')
def eng():
    from cor_asv_ann_amd.engine import HipEngine
    e = HipEngine(1, 32, 8)
    yield e
    e.close()


def _bits_range(lo, hi, step=1):
    """Every `step`-th float32 in [lo, hi] (lo, hi >= 0), by bit pattern."""
    a, b = np.array([lo, hi], np.float32).view(np.uint32)
    return np.arange(a, b + 1, step, dtype=np.uint32).view(np.float32)


def _specials():
    f = np.finfo(np.float32)
    tiny = np.float32(np.nextafter(np.float32(0), np.float32(1)))
    v = [0.0, tiny, f.tiny, f.max, np.inf, 1e3, 1e10, 88.0, 89.0, 0.25, np.nextafter(np.float32(0.25), np.float32(0))]
    v = np.array(v, np.float32)
    return np.concatenate([v, -v, np.array([np.nan], np.float32)])


def _inputs():
    pos = np.concatenate([_bits_range(0.0, 30.0, 64),             # every 64th bit pattern with |x| <= 30
                          _bits_range(0.2499, 0.2501),             # the Taylor branch's switch
                          _bits_range(8.5, 9.5),                   # tanh reaches 1 in float32
                          _bits_range(16.0, 17.5),                 # sigmoid reaches 1
                          _bits_range(87.0, 104.5)])               # sigmoid(-x): subnormal results, then 0
    return np.concatenate([pos, -pos, _specials()])


def _ref(which, x):
    x = x.astype(np.float64)
    with np.errstate(over='ignore'):
        return np.tanh(x) if which == 'tanh' else 1.0 / (1.0 + np.exp(-x))


@pytest.mark.parametrize('which', ['tanh', 'sigmoid'])
def test_activation_within_bound_of_float64(eng, which):
    x = _inputs()
    y = eng.debug_activation(which, x)
    num = ~np.isnan(x)
    assert np.isnan(y[~num]).all()                               # NaN in -> NaN out
    assert not np.isnan(y[num]).any()
    err = np.abs(y[num].astype(np.float64) - _ref(which, x[num]))
    i = int(err.argmax())
    assert err[i] <= ACT_BOUND, (which, float(x[num][i]), float(err[i]))
    inf = np.array([np.inf, -np.inf], np.float32)
    yi = eng.debug_activation(which, inf)
    if which == 'tanh':
        assert yi.tolist() == [1.0, -1.0]
    else:
        assert yi.tolist() == [1.0, 0.0]
        assert (y[num] >= 0).all() and (y[num] <= 1).all()


def test_tanh_is_odd_bit_for_bit(eng):
    x = _inputs()
    x = x[~np.isnan(x)]
    a, b = eng.debug_activation('tanh', x), eng.debug_activation('tanh', -x)
    assert np.array_equal((-a).view(np.uint32), b.view(np.uint32))


def test_lstm_cell_within_bound_of_float64(eng):
    rng = np.random.default_rng(3)
    n = 1 << 20
    z = rng.uniform(-12, 12, (n, 4))
    z[::4] *= 0.03                                      # every 4th row inside the Taylor branch of fast_tanh
    cprev = rng.uniform(-20, 20, (n, 1))
    cprev[1::4] *= 0.01
    x = np.concatenate([z, cprev], axis=1).astype(np.float32)
    got = eng.debug_activation('lstm_cell', x).astype(np.float64)
    zi, zf, zg, zo, cp = (x[:, k].astype(np.float64) for k in range(5))
    sg = lambda v: 1.0 / (1.0 + np.exp(-v))
    i, f, g, o = sg(zi), sg(zf), np.tanh(zg), sg(zo)
    c = f * cp + i * g
    h = o * np.tanh(c)
    # c = fma(f, c_prev, i*g): each activation within ACT_BOUND, plus two roundings of the products; h = o * tanh(c): both
    # activations, the error of c (|d tanh| <= 1, o <= 1) and one rounding
    eps = 2.0 ** -24
    bc = ACT_BOUND * (np.abs(cp) + 2) + 2 * eps * (np.abs(f * cp) + np.abs(i * g)) + 1e-12
    bh = 2 * ACT_BOUND + bc + 2 * eps * np.abs(h)
    assert (np.abs(got[:, 0] - c) <= bc).all(), float((np.abs(got[:, 0] - c) / bc).max())
    assert (np.abs(got[:, 1] - h) <= bh).all(), float((np.abs(got[:, 1] - h) / bh).max())
