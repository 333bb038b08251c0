"""Largest absolute error of the inline activations (csrc/common.h) against float64 over the inputs of
tests/test_gpu_activations.py, and where it occurs.
    python profiles/activation_error.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.test_gpu_activations import _inputs, _ref  # noqa: E402
from cor_asv_ann_amd.engine import HipEngine  # noqa: E402

eng = HipEngine(1, 32, 8)
x = _inputs()
x = x[~np.isnan(x)]
for which in ('tanh', 'sigmoid'):
    err = np.abs(eng.debug_activation(which, x).astype(np.float64) - _ref(which, x))
    i = int(err.argmax())
    small = np.abs(x) < 0.25
    print('%-8s max_abs_error %.4g at x = %.9g; |x| < 0.25: %.4g; |x| >= 0.25: %.4g'
          % (which, err[i], x[i], err[small].max(), err[~small].max()))
eng.close()
