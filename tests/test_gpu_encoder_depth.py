"""The encoder at depths 6 and 8, on a real MI355X.  The per-step form runs layers 2..D as a wavefront in groups of GEMM_MAX_JOBS = 4
layers per launch (csrc/encoder.hip, run_wavefront): a second group exists only from depth 6 on -- at depth 6 it is a single layer,
at depth 8 (the depth limit) three.  33 lines make a second 32-row block (persist_split.hip) and a third 16-row block
(persist.hip) of one row each.  Per-step and persistent forms against the oracle at the tolerances of tests/test_gpu_topology.py
(the oracle's own float32-against-float64 difference on these inputs is below 0.2 % of them), and against each other bit for bit,
in both arithmetics."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import ModelConfig, make_weights, make_lines, vectorize_lines
from oracle.decode import OracleModel

RT, AT = 2e-4, 2e-6
WIDTH, V, LENGTH, EMB_SCALE = 32, 48, 9, 12.0


@functools.lru_cache(maxsize=None)
def _case(depth, B):
    cfg = ModelConfig(depth=depth, width=WIDTH, voc_size=V)
    weights = make_weights(cfg, emb_scale=EMB_SCALE)
    lines, idx = make_lines(B, LENGTH, 11, voc_size=V)
    om = OracleModel(cfg, weights)
    enc_in, _, _, _ = vectorize_lines(om, lines, [[] for _ in lines])
    want = om.encode(enc_in)
    return cfg, weights, idx, np.asarray(want[0]), np.stack(want[1:-1])


@pytest.mark.parametrize('arithmetic', [0, 2])
@pytest.mark.parametrize('depth,B', [(6, 5), (8, 33)])
def test_second_wavefront_group_equals_the_oracle_and_the_persistent_form(depth, B, arithmetic):
    from cor_asv_ann_amd.engine import HipEngine
    cfg, weights, idx, want_enc, want_states = _case(depth, B)
    eng = HipEngine(cfg.depth, cfg.width, cfg.voc_size)
    eng.set_weights(weights)
    eng.set_option('arithmetic', arithmetic)
    outs = []
    for persistent in (0, 1):
        eng.set_option('persistent', persistent)
        eng.encode(idx)
        enc, states = eng.encoder_outputs()
        states = np.stack(states)
        assert eng.stat('encoder_persistent') == persistent
        assert np.allclose(enc, want_enc, rtol=RT, atol=AT), persistent
        assert np.allclose(states, want_states, rtol=RT, atol=AT), persistent
        outs.append((enc, states))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    eng.close()
