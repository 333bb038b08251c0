"""The references and bounds of tests/test_gpu_score.py hold on the CPU: the two oracles agree on the exact outputs, the stepped
restatement is the training graph's forward pass (where it can be), the float32 reference's own error is what the device bound
is built on, the checks catch four wrong heads, and the facade's score_lines does its bookkeeping on a stub engine."""
import numpy as np
import pytest

from tests import score_cases as sc


# ------------------------------------------------------------------------------------------------ 1. the exact outputs are well defined
@pytest.mark.parametrize('c', sc.MODEL_CASES, ids=sc.IDS)
def test_both_oracles_pick_the_same_best_and_rank(c):
    """The GPU test may leave out the positions where the fp32 and the fp64 oracle differ, at most 2 % of a case's; on these cases
    there is none."""
    o = sc.oracles(c)
    assert o['agree'].mean() >= 0.98
    assert o['agree'].all()
    top2 = np.sort(o['P64'], axis=2)[:, :, -2:]
    assert ((top2[:, :, 1] - top2[:, :, 0]) / top2[:, :, 1]).min() > 1e-4        # (no near-tie a rounding could turn)


# ------------------------------------------------------------------------------------------------ 2. the stepped restatement
@pytest.mark.parametrize('c', [c for c in sc.MODEL_CASES if 'residual_connections' not in c[6]],
                         ids=[i for c, i in zip(sc.MODEL_CASES, sc.IDS) if 'residual_connections' not in c[6]])
def test_stepped_restatement_is_the_training_forward(c):
    mc, o = sc.model_case(c), sc.oracles(c)
    P, rows = sc.stepped(mc['cfg'], mc['w'], mc['enc_in'], mc['dec_in'])
    assert np.abs(P - o['P32']).max() <= 7.5e-8
    assert rows.shape == mc['dec_in'].shape[:2] + (mc['enc_in'].shape[1],) and np.allclose(rows.sum(axis=2), 1, atol=1e-5)
    P64 = sc.stepped(mc['cfg'], {k: v.astype(np.float64) for k, v in mc['w'].items()}, mc['enc_in'], mc['dec_in'], np.float32)[0]
    assert np.abs(P64 - o['P64']).max() <= 1e-12


def test_stepped_restatement_is_refused_with_residual_connections():
    c = [c for c in sc.MODEL_CASES if 'residual_connections' in c[6]][0]
    mc, o = sc.model_case(c), sc.oracles(c)
    assert o['rows64'] is None
    with pytest.raises(ValueError):
        sc.stepped(mc['cfg'], mc['w'], mc['enc_in'], mc['dec_in'])
    # ... because the reference's inference decoder has no residual sums: its probabilities are another model's
    cfg = sc.ModelConfig(depth=c[0], width=c[1], voc_size=c[2], bridge_dense=True)
    P = sc.stepped(cfg, mc['w'], mc['enc_in'], mc['dec_in'])[0]
    assert np.abs(P - o['P32']).max() > 0.1


# ------------------------------------------------------------------------------------------------ 3. the reference's own float32 error
def test_float32_head_error_in_units():
    e = sc.e_np()
    print('E_np = %.3f units of 2^-24 (|logp64| + 1)' % e)
    assert 0 < e <= 2
    x, t = sc.head_case(4096, 80.0)
    assert sc.head64(x, t)[0].min() < -300              # (most exponentials underflow at this scale)


def test_both_heads_agree_on_the_exact_outputs():
    for V in sc.HEAD_V:
        for s in sc.HEAD_SCALES:
            x, t = sc.head_case(V, s)
            a, b = sc.head32(x, t), sc.head64(x, t)
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
            assert {0, V - 1, -1} <= set(t.tolist())
    for name, x, t in sc.constructed_rows():
        a, b = sc.head32(x[None], [t]), sc.head64(x[None], [t])
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), name
        assert np.array_equal(a[0], b[0].astype(np.float32), equal_nan=True) or sc.units(a[0], b[0]).max() <= 2, name


def test_constructed_rows_say_what_their_names_say():
    rows = {name: sc.head64(x[None], [t]) + (x, t) for name, x, t in sc.constructed_rows()}
    lp, b, r, x, t = rows['all_equal']
    assert b[0] == 0 and r[0] == 0 and abs(lp[0] + np.log(len(x))) < 1e-12
    for name, (lp, b, r, x, t) in rows.items():
        if name.startswith('tie_'):
            ties = [int(v) for v in name.split('_')[2:-1]]
            assert b[0] == ties[0] and (r[0] == 0 if t in ties else r[0] >= len(ties)), name     # (strict: the tie's own entries do not count)
        if name.startswith('nan_at') or name in ('plus_inf', 'all_minus_inf'):
            assert np.isnan(lp[0]) and b[0] == -1 and r[0] == -1, name
    lp, b, r, x, t = rows['minus_inf_at_target']
    assert lp[0] == -np.inf and r[0] == len(x) - 1 and b[0] >= 0
    lp, b, r, x, t = rows['minus_inf_unscored']
    assert lp[0] == 0 and r[0] == -1 and b[0] >= 0


# ------------------------------------------------------------------------------------------------ 4. the checks can fail
def _checks(got, x, t):
    """The GPU test's checks of the head on one batch of rows: (logp excess over its bound of 4 E_np units, best exact, rank exact)."""
    lp, b, r = sc.head64(x, t)
    return float(sc.units_or_inf(got[0], lp).max(initial=0.0)) / (4 * sc.e_np()), np.array_equal(got[1], b), np.array_equal(got[2], r)


def test_four_mistakes_leave_the_bounds():
    named = {name: (x[None], np.array([t], np.int32)) for name, x, t in sc.constructed_rows()}
    # a padding column read: the row of negative logits, padding 0 -- the maximum, the sum and the rank see the padding
    x, t = named['negative_only']
    excess, best_ok, rank_ok = _checks(sc.MISTAKES['padding_column_read'](x, t, 0.0), x, t)
    assert excess >= 10 and not rank_ok
    assert _checks(sc.MISTAKES['padding_column_read'](x, t, np.nan), x, t)[0] == np.inf
    # >= in the rank: the target inside a tie
    x, t = named['tie_40_3_9_t9']
    excess, best_ok, rank_ok = _checks(sc.MISTAKES['rank_counts_ties'](x, t, 0.0), x, t)
    assert excess <= 1 and best_ok and not rank_ok
    # the highest index on an argmax tie, across lanes and across a lane's passes
    for name in ('tie_96_5_69_t1', 'tie_640_69_581_t1', 'all_equal'):
        x, t = named[name]
        excess, best_ok, rank_ok = _checks(sc.MISTAKES['argmax_takes_the_last'](x, t, 0.0), x, t)
        assert excess <= 1 and not best_ok and rank_ok, name
    # the loss's clip on logp: at scale 80 log p reaches -500, the clip stops at log 1e-7
    x, t = sc.head_case(640, 80.0)
    assert _checks(sc.MISTAKES['loss_clip_on_logp'](x, t, 0.0), x, t)[0] >= 10
    # ... and the right head passes all of them
    for x, t in list(named.values()) + [sc.head_case(640, 80.0)]:
        excess, best_ok, rank_ok = _checks(sc.head32(x, t), x, t)
        assert excess <= 1 and best_ok and rank_ok


# ------------------------------------------------------------------------------------------------ 5. the facade on a stub engine
class _StubEngine(object):
    """score_targets with made-up values that encode (call, row, position), and a record of the calls."""
    def __init__(self):
        self.calls = []
        self.T = 999

    def score_targets(self, idx, val, dec_in, dec_out, want_align=False):
        B, U = dec_out.shape
        T = idx.shape[1]
        k = len(self.calls)
        self.calls.append((idx.copy(), dec_in.copy(), dec_out.copy(), want_align))
        logp = -(100.0 * k + 10.0 * np.arange(B)[:, None] + np.arange(U)[None, :]).astype(np.float32)
        logp[dec_out < 0] = 0
        best = np.where(dec_out >= 0, dec_out, 5).astype(np.int32)
        best[0, 0] = -1                                     # an invalid row
        rank = np.where(dec_out >= 0, np.arange(U)[None, :], -1).astype(np.int32)
        count = (dec_out >= 0).sum(axis=1).astype(np.int32)
        nll = -logp.astype(np.float64).sum(axis=1)
        align = None
        if want_align == 'sparse':
            align = (np.zeros((B, U), np.int32), np.full((B, U, 11), 1 / 11, np.float32))
        elif want_align:
            align = np.full((B, U, T), 1.0 / T, np.float32)
        return logp, best, rank, nll, count, align


def _stub_facade(batch_size):
    from cor_asv_ann_amd.seq2seq import Sequence2Sequence
    from oracle import make_vocabulary
    s2s = Sequence2Sequence()
    s2s.depth, s2s.width, s2s.batch_size = 1, 32, batch_size
    s2s.mapping, s2s.voc_size = make_vocabulary(100), 100
    s2s.engine = _StubEngine()
    s2s._require_engine = lambda: s2s.engine
    s2s.status = 2
    return s2s


def test_score_lines_bookkeeping_on_a_stub_engine():
    from cor_asv_ann_amd.realign import SparseAlignment
    s2s = _stub_facade(2)
    sources = ['abc\n', 'de\n', 'fgh\n', '', 'ij\n']
    targets = ['abd\n', '', 'fg\n', 'xy\n', 'ijkl\n']
    logprobs, scores, predictions, ranks, aligns = s2s.score_lines(sources, targets)
    calls = s2s.engine.calls
    assert len(calls) == 2 and [c[2].shape for c in calls] == [(2, 5), (1, 6)] and calls[0][3] is False     # pairs 0, 2 | 4; U = longest + 1
    for j in (1, 3):                                        # skipped as evaluate skips them
        assert (logprobs[j], scores[j], predictions[j], ranks[j], aligns[j]) == ([], 0.0, '', [], [])
    assert [len(x) for x in logprobs] == [4, 0, 3, 0, 5] == [len(x) for x in ranks]
    assert logprobs[2] == [-10.0, -11.0, -12.0] and logprobs[4] == [-100.0, -101.0, -102.0, -103.0, -104.0]
    assert scores[2] == 11.0 and scores[4] == 102.0 and scores[0] == 1.5
    assert predictions == ['bd\n', '', 'fg\n', '', 'jkl\n']            # (-1 becomes no character)
    assert ranks[4] == [0, 1, 2, 3, 4] and all(isinstance(v, int) for v in ranks[4]) and all(isinstance(v, float) for v in logprobs[4])
    assert aligns == [[], [], [], [], []]
    c_i = s2s.mapping[0]
    assert calls[0][2][1].tolist() == [c_i['f'], c_i['g'], c_i['\n'], -1, -1] and calls[0][1][1].tolist() == [-1, c_i['f'], c_i['g'], c_i['\n'], -1]
    al = s2s.score_lines(sources, targets, alignments=True)[4]
    assert s2s.engine.calls[-1][3] == 'sparse' and isinstance(al[0], SparseAlignment) and len(al[0]) == 4 and al[1] == []
    assert np.asarray(al[4]).shape == (5, 3)                # T of the pair's own chunk, not the engine's last decode
    al = s2s.score_lines(sources, targets, alignments='dense')[4]
    assert s2s.engine.calls[-1][3] is True and len(al[2]) == 3 and al[2][0].shape == (4,) and al[3] == []
    assert s2s.score_lines([], []) == ([], [], [], [], [])
    s2s.status = 1
    with pytest.raises(AssertionError):
        s2s.score_lines(sources, targets)
