"""The training state's small cases (tests/test_gpu_train_state.py, profiles/train_state_bits.py): the four topologies whose
Keras <-> packed tables differ -- depth 1, depth 2, depth 2 with a deep bidirectional encoder, depth 2 with bridge_dense -- at
W = 32, V = 7 with a batch of B = 2, T = U = 3, A = 1."""
import numpy as np

from oracle import ModelConfig, make_weights

W, V, B, T, U = 32, 7, 2, 3, 3
CONFIGS = (('d1', 1, {}), ('d2', 2, {}), ('d2_deep', 2, dict(deep_bidirectional_encoder=True)), ('d2_bridge', 2, dict(bridge_dense=True)))
IDS = [c[0] for c in CONFIGS]


def weights_of(depth, width, voc, flags, seed=11):
    """make_weights with every bias drawn too (a zero or constant bias would hide a permuted one)."""
    w = make_weights(ModelConfig(depth=depth, width=width, voc_size=voc, **flags), emb_scale=4.0)
    rng = np.random.default_rng(seed)
    for k in w:
        if w[k].ndim == 1:
            w[k] = (w[k] + rng.normal(size=w[k].shape) * 0.2).astype(np.float32)
    return w


def batch_of(voc, b, t, u, seed=5):
    """(enc_idx (b,t), None, dec_in (b,u), dec_out (b,u), weights (b,u)) of random characters, every position counted."""
    rng = np.random.default_rng(seed)
    return (rng.integers(2, voc, (b, t)).astype(np.int32), None, rng.integers(2, voc, (b, u)).astype(np.int32),
            rng.integers(1, voc, (b, u)).astype(np.int32), np.ones((b, u), np.float32))


def soft_of(voc, b, u, k=2, seed=6):
    """K distinct (index, mass) slots per position, masses summing to 1."""
    rng = np.random.default_rng(seed)
    idx = np.stack([rng.permutation(np.arange(1, voc))[:k] for _ in range(b * u)]).reshape(b, u, k).astype(np.int32)
    q = rng.random((b, u, k)).astype(np.float32) + 0.1
    return idx, (q / q.sum(axis=2, keepdims=True)).astype(np.float32)


def distinct(shape, start):
    """An all-distinct float32 tensor: start, start + 1, ... (exact below 2^24)."""
    return (np.arange(int(np.prod(shape)), dtype=np.float32) + np.float32(start)).reshape(shape)
