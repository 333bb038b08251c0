"""Everything the decode entry points return, dumped for a byte-for-byte comparison of two builds of the library (the split of
the decode host code into a step view and phases must change no bit).

    CASV_LIB_PATH=<build A's libcor_asv_ann_hip.so> python profiles/decode_phases_equality.py dump a.npz
    CASV_LIB_PATH=<build B's>                       python profiles/decode_phases_equality.py dump b.npz
    python profiles/decode_phases_equality.py compare a.npz b.npz profiles/decode_phases_equality.json

Models: width 64, 48 characters, depths 1, 2, 3 and a bridge_dense model; 21 ragged lines on 12 positions (one of length 1).
Greedy modes 0 and 1 x persistent 0 / 1 x graph 0 / 1 x with / without alignments, and with pin_limit_mb 0; beam N = 4 (and
N = 128 on 3 lines, which skips dead rows from the first step) x lm_predict x graph x max_results 1 / 3 over 40 steps (several
chunks, an early stop); the explicit decoder step with and without the LM output; sparse alignments and result records behind a
greedy and a beam call; a beam call then a greedy call on one handle; one beam call behind the injected encoder give-up."""
import json
import os
import sys

os.environ.setdefault('CASV_FAULT_INJECTION', '1')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

W, V, B, T = 64, 48, 21, 12
BEAM_KEYS = ('idx', 'prob', 'score', 'len', 'align', 'rej', 'n_found', 'n_steps')
MODELS = {'d1': (1, {}), 'd2': (2, {}), 'd3': (3, {}), 'bridge': (2, dict(bridge_dense=True))}


def lines(n, seed=5, alts=3):
    """n confusion-network lines of mixed length: line 0 has all T positions, line 1 the end of line alone."""
    rng = np.random.default_rng(seed)
    idx = np.full((n, T, alts), -1, np.int32)
    val = np.zeros((n, T, alts), np.float32)
    for j in range(n):
        length = T if j == 0 else 1 if j == 1 else int(rng.integers(1, T + 1))
        for t in range(length - 1):
            k = int(rng.choice([1, 2, 3], p=[0.60, 0.28, 0.12]))
            idx[j, t, :k] = rng.choice(np.arange(2, V), size=k, replace=False)
            val[j, t, :k] = np.sort(rng.dirichlet(np.ones(k) * 0.7) * rng.uniform(0.7, 1.0))[::-1]
        idx[j, length - 1, 0], val[j, length - 1, 0] = 1, 1.0
    return idx, val


def dump(path):
    from oracle import ModelConfig, make_weights
    from cor_asv_ann_amd.engine import HipEngine
    import cor_asv_ann_amd._native as nv
    out = {}

    def keep(tag, arrays):
        for k, a in enumerate(arrays):
            if a is not None:
                out['%s/%d' % (tag, k)] = np.ascontiguousarray(a)

    def options(eng, **kw):
        for k, v in kw.items():
            eng.set_option(k, v)

    full, few = lines(B), lines(3, seed=6)
    for name, (depth, flags) in MODELS.items():
        cfg = ModelConfig(depth=depth, width=W, voc_size=V, **flags)
        weights = make_weights(cfg, emb_scale=8.0)
        eng = HipEngine(depth, W, V, **flags)
        eng.set_weights(weights)

        def greedy(tag, mode, align, batch=full):
            """Through the C ABI itself: mode 1 on these weights meets an all-NaN row before some line's end, which the facade
            raises (CASV_ERR_NAN, -5) -- the arrays have been written by then and are part of the comparison, with the status."""
            eng.encode(*batch)
            n, S = batch[0].shape[0], 2 * T
            idx, prob, length = np.zeros((n, S), np.int32), np.zeros((n, S), np.float32), np.zeros((n,), np.int32)
            al = np.zeros((n, S, T), np.float32) if align else None
            rc = eng.lib.casv_decode_greedy(eng.handle, mode, S, nv.ptr(idx), nv.ptr(prob), nv.ptr(length), nv.ptr(al))
            if rc != -5:
                nv.check(rc)
            keep(tag, [idx, prob, length, al, np.array([rc], np.int32)])

        def beam(tag, batch=full, **kw):
            eng.encode(*batch)
            res = eng.decode_beam(rejection_threshold=0.5, steps=40, **kw)
            keep(tag, [res[k] for k in BEAM_KEYS])

        for mode in (0, 1):
            for persistent in (0, 1):
                for graph in (0, 1):
                    for align in (False, True):
                        options(eng, persistent=persistent, graph=graph)
                        greedy('%s/greedy/m%d/p%d/g%d/a%d' % (name, mode, persistent, graph, align), mode, align)
                options(eng, persistent=persistent, graph=0, pin_limit_mb=0)        # results straight to the caller's arrays
                greedy('%s/greedy/m%d/p%d/unstaged' % (name, mode, persistent), mode, True)
                options(eng, pin_limit_mb=64)
        options(eng, persistent=0, graph=0)
        greedy(name + '/greedy/then', 0, False)
        keep(name + '/greedy/sparse', eng.alignments_sparse(B, 2 * T))
        eng.records_reset(B + 2, 2 * T)
        eng.records_append(1)
        keep(name + '/greedy/records', [eng.records_read()])
        for lm in (0, 1):
            for graph in (0, 1):
                options(eng, lm_predict=lm, graph=graph, persistent=-1)
                for mr in (1, 3):
                    beam('%s/beam/lm%d/g%d/mr%d' % (name, lm, graph, mr), batch_size=4, max_results=mr, want_align=True)
                beam('%s/beam/lm%d/g%d/noalign' % (name, lm, graph), batch_size=4)
                beam('%s/beam128/lm%d/g%d' % (name, lm, graph), batch=few, batch_size=128, want_align=True)
        options(eng, lm_predict=0, graph=0)
        beam(name + '/beam/then', batch_size=4, max_results=3)
        keep(name + '/beam/sparse', eng.alignments_sparse(3 * B, 40))
        eng.records_reset(B, 40)
        eng.records_append(0)
        keep(name + '/beam/records', [eng.records_read()])
        # a wide search (live rows handed to the step from its first iteration), then a greedy decode on the same handle
        options(eng, persistent=0)
        beam(name + '/mixed/beam128', batch=few, batch_size=128)
        greedy(name + '/mixed/greedy', 1, True, batch=few)
        # the explicit step, on the states the encoder leaves
        eng.encode(*full)
        enc, states = eng.encoder_outputs()
        p_in = np.zeros((B, V), np.float32)
        p_in[np.arange(B), 2 + np.arange(B) % (V - 2)] = 1.0
        a_in = np.zeros((B, T), np.float32)
        row = np.arange(B, dtype=np.int32)
        probs, st = eng.decoder_step(row, p_in, states, a_in)
        keep(name + '/step', [probs] + st)
        probs, lm_probs, st = eng.decoder_step_lm(row[::-1].copy(), p_in, states, a_in)
        keep(name + '/step_lm', [probs, lm_probs] + st)
        eng.close()
    # the encoder's give-up, injected once: the search starts over on the pass redone per step
    cfg = ModelConfig(depth=2, width=W, voc_size=V)
    eng = HipEngine(2, W, V)
    eng.set_weights(make_weights(cfg, emb_scale=8.0))
    eng.set_option('persistent', 3)
    eng.encode(*full)
    res = eng.decode_beam(batch_size=4, want_align=True)
    keep('give_up/beam', [res[k] for k in BEAM_KEYS] + [np.array([eng.stat('encoder_persistent')])])
    eng.close()
    np.savez(path, **out)
    print('dumped %d arrays, %d bytes' % (len(out), sum(a.nbytes for a in out.values())))


def compare(a_path, b_path, json_path):
    a, b = np.load(a_path), np.load(b_path)
    mismatches = sorted(set(a.files) ^ set(b.files))
    nbytes = 0
    for k in sorted(set(a.files) & set(b.files)):
        x, y = a[k], b[k]
        nbytes += x.nbytes
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            mismatches.append(k)
    paragraphs = [x.replace('\n', ' ') for x in __doc__.split('\n\n')]
    result = {'what': paragraphs[0], 'cases': paragraphs[2], 'arrays': len(a.files), 'bytes': nbytes, 'mismatches': mismatches}
    with open(json_path, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps({k: result[k] for k in ('arrays', 'bytes', 'mismatches')}))
    return 1 if mismatches else 0


if __name__ == '__main__':
    sys.exit(dump(sys.argv[2]) if sys.argv[1] == 'dump' else compare(*sys.argv[2:5]))
