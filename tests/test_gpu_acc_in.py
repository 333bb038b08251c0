"""GemmArgs.acc_in (csrc/gemm_args.h) on a real MI355X: a contraction over [x | h] in ONE launch against the x columns alone
(no bias: the raw accumulators) followed by the h columns on top of them, bit for bit -- the property the encoder's per-character
table (csrc/encoder.hip, tests/test_gpu_encoder_table.py) rests on.

Both runs are the same instruction sequence per element: x comes first in K, the cut falls between two K tiles, and between two
matrix instructions an accumulator is a plain fp32 register value.  So there is no tolerance: every comparison is of the bits.
The x part is produced once as 128x128 split tiles (arithmetic 1) and once as 256x256 tiles (arithmetic 2, M = 16384 rows so that
the job fills the chip that way); the accumulator rows are gathered through an index that repeats rows and includes the zero row.
"""
import numpy as np
import pytest

from tests.lstm_gemm_cases import FORM_BITS, Job, Part

pytestmark = pytest.mark.gpu

N = 512
POOL = 200              # rows of the x pool the jobs gather from; the last one is the zero row ("no character")
BIG = 16384             # rows of the x contraction that runs as 256x256 tiles: 64 x 2 tiles >= 128


@pytest.fixture(scope='module')
def engine():
    from cor_asv_ann_amd.engine import HipEngine
    eng = HipEngine(1, 32, 8)
    try:
        yield eng
    finally:
        eng.set_option('split_bf16', -1)
        eng.close()


_x_parts = {}


def x_part(eng, kx, tiles):
    """-> (X (POOL, kx), Bx (N, kx), Ax (POOL, N)): the x pool, the x columns of the weight, and the raw accumulators of X . Bx^T from
    a launch of 128x128 (tiles = 1) or 256x256 (tiles = 2) split tiles.  Computed once per (kx, tiles)."""
    if (kx, tiles) in _x_parts:
        return _x_parts[kx, tiles]
    rng = np.random.default_rng(1000 + kx)
    X = rng.standard_normal((BIG, kx)).astype(np.float32)
    X[POOL - 1] = 0.0
    Bx = (rng.standard_normal((N, kx)) / np.sqrt(kx)).astype(np.float32)
    rows = POOL if tiles == 1 else BIG
    ktot = max(kx, 32)
    Bt = np.zeros((N, ktot), np.float32)
    Bt[:, :kx] = Bx
    job = Job(M=rows, N=N, Ktot=ktot, segs=[Part(X[None, :rows], kx, step_mul=0)], Bt=Bt, out=(1, N, 0, 0))
    eng.set_option('split_bf16', tiles)
    res, forms, launches = eng.debug_gemm_jobs(0, [job], 0, acc=[None])
    want = FORM_BITS['s256'] if tiles == 2 else FORM_BITS['s128']
    assert forms == 1 << want and launches == 1, (forms, launches)
    Ax = res[0]['out'][0, :POOL].copy()
    assert not Ax[POOL - 1].any() and not np.signbit(Ax[POOL - 1]).any()        # the zero row: +0 accumulators
    _x_parts[kx, tiles] = (X[:POOL].copy(), Bx, Ax)
    return _x_parts[kx, tiles]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize('arithmetic', [1, 2])
@pytest.mark.parametrize('tiles', [1, 2])
@pytest.mark.parametrize('kx', [16, 32, 512])
def test_x_then_h_on_its_accumulators_equals_the_undivided_contraction(engine, kx, tiles, arithmetic):
    X, Bx, Ax = x_part(engine, kx, tiles)
    engine.set_option('split_bf16', arithmetic)
    for M in (128, 256, 130):
        for kh in (0, 16, 512):
            for lstm in (False, True):
                rng = np.random.default_rng([M, kh, kx, int(lstm)])
                khw = kh or 16                      # (kh = 0: the h segment is dropped by skip_first at step 0)
                step = 1 if kh else 0
                idx = rng.integers(0, POOL, M).astype(np.int32)
                idx[1] = idx[0]; idx[M - 1] = idx[0]            # rows that repeat, within a wave's rows and across tiles
                idx[2] = POOL - 1; idx[M - 2] = POOL - 1        # the zero row
                ktot = kx + khw
                Bt = np.empty((N, ktot), np.float32)
                Bt[:, :kx] = Bx
                Bt[:, kx:] = (rng.standard_normal((N, khw)) / np.sqrt(khw)).astype(np.float32)
                bias = rng.standard_normal(N).astype(np.float32)
                H = rng.standard_normal((2, M, khw)).astype(np.float32)
                C = rng.standard_normal((2, M, N // 4)).astype(np.float32)

                def job(segs):
                    kw = dict(M=M, N=N, Ktot=ktot, segs=segs, Bt=Bt, bias=bias)
                    if lstm:
                        kw.update(out=(2, N // 4, 1, 0), c_in=Part(C, N // 4), c_out=(2, N // 4, 1, 0))
                    else:
                        kw.update(out=(2, N, 1, 0))
                    return Job(**kw)
                h_seg = Part(H, khw, koff=kx, skip_first=True)
                whole = job([Part(X[None], kx, rows=idx, step_mul=0), h_seg])
                on_top = job([h_seg])
                want, forms_w, _ = engine.debug_gemm_jobs(int(lstm), [whole], step, acc=[None])
                got, forms_g, launches = engine.debug_gemm_jobs(int(lstm), [on_top], step, acc=[Part(Ax[None], N, rows=idx, step_mul=0)])
                assert forms_w == forms_g == 1 << FORM_BITS['s128'] and launches == 1
                for name in want[0]:
                    a, b = bits(want[0][name][step]), bits(got[0][name][step])
                    bad = np.argwhere(a != b)
                    assert not len(bad), 'M=%d kx=%d kh=%d lstm=%d %s: %d elements differ, first at %s' % (M, kx, kh, lstm, name, len(bad), bad[0])
                    assert np.isfinite(got[0][name][step]).all()


def test_acc_in_is_refused_outside_the_split_tiles(engine):
    """Arithmetic 0 has no form that reads the field: the entry point says so instead of launching."""
    from cor_asv_ann_amd import _native as nv
    X, Bx, Ax = x_part(engine, 32, 1)
    engine.set_option('split_bf16', 0)
    M = 128
    job = Job(M=M, N=N, Ktot=32, segs=[Part(X[None, :M], 32, step_mul=0)], Bt=Bx, out=(1, N, 0, 0))
    with pytest.raises(nv.NativeError):
        engine.debug_gemm_jobs(0, [job], 0, acc=[Part(Ax[None], N, step_mul=0)])
