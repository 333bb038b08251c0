"""The Keras <-> packed table of the training state (csrc/keras_table.h) on the host: tests/keras_table_check.cpp, built with the
address and undefined-behaviour sanitizers, round-trips every entry of four topologies; its entries are weight_shapes()'s tensors."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from cor_asv_ann_amd.engine import weight_shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {'depth 1': (1, {}), 'depth 2': (2, {}), 'depth 2, deep_bidirectional_encoder': (2, dict(deep_bidirectional_encoder=True)),
           'depth 2, bridge_dense': (2, dict(bridge_dense=True))}


def test_every_entry_round_trips_and_no_two_overlap(tmp_path):
    cxx = os.environ.get('CXX') or next((c for c in ('c++', 'g++', 'clang++') if shutil.which(c)), None)
    if not cxx or not shutil.which(cxx):
        pytest.skip('no host compiler')
    exe = str(tmp_path / 'keras_table_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Werror',
                    os.path.join(ROOT, 'tests', 'keras_table_check.cpp'), '-o', exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    tables, name = {}, None
    for line in run.stdout.splitlines():
        if line.startswith('  '):
            tensor, rows, cols = line.split()
            tables[name][tensor] = int(rows) * int(cols)
        else:
            name = line.split(':')[0]
            assert line.endswith(': ok'), line
            tables[name] = {}
    assert set(tables) == set(CONFIGS)
    for name, (depth, flags) in CONFIGS.items():
        want = {k: int(np.prod(s)) for k, s in weight_shapes(depth, 32, 7, **flags).items()}
        assert tables[name] == want, name
