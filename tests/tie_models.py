"""Models whose distributions are exactly tied, and the table of searches run on them -- test infrastructure, importable
without a GPU (tests/test_tie_models.py on the CPU, tests/test_gpu_beam_ties.py on the device).

On such a model the result of the best-first search is decided by its bookkeeping rules alone (csrc/beam_kernels.hip, head
comment; oracle/decode.py decode_sequence_beam): candidate order inside a row (score descending, ties towards the HIGHER index),
queue order (pro_cost descending, among equals the node created first: `insort_left` + `pop()`), the queue cap 2*T*N taken from
the popping end, the strict `>` of the stop test, where beam_width_in / beam_threshold_in cut a row, the skip of index 0 and the
rejection candidate behind the beam.

Two families, both made from `oracle.make_weights` by overwriting entries:

uniform     every tensor zero.  h = c = 0, logits 0, every probability fl32(1/V); attention energies exp(0) = 1, so alignments
            are fl32(1/n) over the window.  Every row is one tie; structure comes from the rejection candidate and the
            successive-reset feedback only.
held state  K, R and the attention tensors zero, encoder biases 0.7; decoder biases 0 on the input and candidate gates, 30 on
            the forget gate, 1 on the output gate: f = fl32(sigmoid(30)) = 1, i * g = 0.5 * tanh(0) = 0, so c, h and the
            distribution keep their bits over all steps of a line.  E is random with its rows duplicated in groups, so that the
            distribution is not uniform and has exact ties inside the groups.  Costs are float32 values summed in float64 --
            exact sums -- so permutations of a multiset of characters tie exactly, on the device and in the oracle alike.

`search` is decode_sequence_beam restated once more with switches for the four order rules (tests/test_tie_models.py shows that
every switch changes an expected output of the table, and that with no switch set it yields what the oracle yields) and with a
trace of what the case table promises: tied pops, cuts inside tie groups, queue and final-list sizes, new keys per step.
"""
from bisect import insort_left, insort_right

import numpy as np

from oracle import ModelConfig, make_weights, make_vocabulary, vectorize_lines
from oracle.decode import Node, OracleModel
from tests.lm_oracle import lm_step

DEPTH, WIDTH = 2, 32
UNMAPPED = '中'            # not in any synthetic vocabulary: index 0 through the reference's lookup (s2s:1078-1083)


# ------------------------------------------------------------------------------------------------------------------ models
def uniform_weights(cfg):
    return {k: np.zeros_like(v) for k, v in make_weights(cfg).items()}


def group_order(V, group, split01):
    """The index order the groups of `group` consecutive entries are cut from.  split01: index 1 ('\\n') is moved behind the first
    group, so that index 0 shares its group with characters and '\\n' opens the second one; otherwise 0 and '\\n' share the first."""
    order = list(range(V))
    if split01 and V > group + 1:
        order = [0] + list(range(2, group + 1)) + [1] + list(range(group + 1, V))
    return order


def groups_of(V, group, split01):
    """index -> group number."""
    g = np.empty(V, np.int64)
    for k, v in enumerate(group_order(V, group, split01)):
        g[v] = k // group
    return g


def held_weights(cfg, group=4, split01=True, boost=0.0, emb_scale=4.0, seed=7):
    """boost: added to every entry of the E rows of '\\n' and its group.  All units of h hold one value (zero K and R, constant
    biases), so a logit is that value times the sum of its E row: the boost makes ending the line the likeliest child."""
    w = make_weights(cfg, seed=seed, emb_scale=emb_scale)
    W, V = cfg.width, cfg.voc_size
    E = w['E'].copy()
    g = groups_of(V, group, split01)
    first = {}
    for v in group_order(V, group, split01):
        first.setdefault(int(g[v]), v)
    for v in range(V):
        E[v] = w['E'][first[int(g[v])]] + (np.float32(boost) if g[v] == g[1] else np.float32(0))
    for k in w:
        if k == 'E':
            w[k] = E
        elif k.startswith('enc') and k.endswith('_b'):
            w[k] = np.full_like(w[k], 0.7)
        elif k.startswith('dec') and k.endswith('_b'):
            b = np.zeros_like(w[k])
            b[W:2 * W] = 30.0           # forget gate: fl32(sigmoid(30)) == 1
            b[3 * W:] = 1.0             # output gate
            w[k] = b
        else:
            w[k] = np.zeros_like(w[k])
    return w


# ------------------------------------------------------------------------------------------------------------------ forms
def beam_form(N, V, width_in, T):
    """The launch form of one search, restated from csrc/beam_kernels.hip:
    beam_lds_bytes (`cm`, `pop_cap = N + 64`, `rows`, the two `while` loops over `cap`, `q_stage`) and launch_beam_step (`vpl`,
    `wide = N >= 8`, `huge = N >= 64`, `split = huge && rowrec` -- casv_decode_beam gives rowrec whenever N >= 64 --, the
    `if (vpl <= 4) ... else` ladder: the 16-wave and split forms exist up to VPL 16 only); q_cap = 2*T*N from casv_decode_beam."""
    cm = min(width_in, V) + 1
    pop_cap = N + 64
    rows = 7 * (N + 1) * 4 + pop_cap * 16
    cap = 1
    while cap < N * cm and cap < 4096:
        cap <<= 1
    while cap > 256 and rows + cap * 12 > 56 * 1024:
        cap >>= 1
    base = rows + cap * 12
    q_cap = 2 * T * N
    q_stage = q_cap if q_cap * 12 + base <= 56 * 1024 else 0
    vpl = (V + 63) // 64
    VPL = 4 if vpl <= 4 else 8 if vpl <= 8 else 16 if vpl <= 16 else 32 if vpl <= 32 else 64
    split = N >= 64 and VPL <= 16
    waves = 16 if split else 8 if N >= 8 else 4
    return dict(VPL=VPL, waves=waves, split=split, sort_cap=cap, q_cap=q_cap, staged=q_stage == q_cap, pop_cap=pop_cap,
                max_new_keys=N * cm)


# ------------------------------------------------------------------------------------------------------------------ search
RULES = ('tie_low', 'insort_right', 'stop_ge', 'cap_other_end')
# ... and of the rejection rule (tests/steer_models.py: models whose attention rows are steered, so that the rule decides)
REJECTION_RULES = ('round_half_up', 'is1_ignored', 'is1_from_attention_row', 'mis_not_tested')
# ... and the threshold of the misalignment moved to either side of 0.1: 0.09 lets a misalignment of 2/21 out, 0.13 lets 1/9 and 1/8 in
THRESHOLD_RULES = ('mis_below_0_09', 'mis_below_0_13')


def search(m, source_seq, encoder_outputs, rules=(), trace=None, lm=False, beyond_line=None):
    """oracle/decode.py decode_sequence_beam, line for line, with
    rules  'tie_low'        candidate ties towards the LOWER index
           'insort_right'   children (and finished hypotheses) inserted behind their equals
           'stop_ge'        `>=` in the stop test
           'cap_other_end'  the queue cap keeps the other end
           'round_half_up'            the source position rounded as floor(x + 0.5) instead of half-to-even
           'is1_ignored'              a one-hot parent alignment treated like any other
           'is1_from_attention_row'   "one-hot" asked of the step's own attention row instead of the parent's alignment
           'mis_not_tested'           the rejection candidate added whatever the misalignment
           'mis_below_0_09', 'mis_below_0_13'   the misalignment compared with 0.09 / 0.13 instead of 0.1
    beyond_line  'no_candidate': a source position beyond the line gives no rejection candidate -- the device's documented
           deviation -- where the reference, and this function without the switch, raise IndexError
    trace  a dict that receives what the case table promises (see the keys below)
    lm     lm_predict: a child's cost comes from the LM's row (tests/lm_oracle.py decode_sequence_beam_lm)
    -> list of (text, probs, score, alignments, rejection positions), best first, and the stats dict."""
    assert set(rules) <= set(RULES + REJECTION_RULES + THRESHOLD_RULES) and beyond_line in (None, 'no_candidate')
    mis_limit = 0.09 if 'mis_below_0_09' in rules else 0.13 if 'mis_below_0_13' in rules else 0.1
    insort = insort_right if 'insort_right' in rules else insort_left
    V = m.voc_size
    i_c = m.mapping[1]
    attended = encoder_outputs[0]
    T = attended.shape[1]
    u = None if m.recompute_u else attended @ m.weights['att_U']
    root = Node(state=list(encoder_outputs[1:]), value='', scores=np.zeros(V), prob=[], cost=0.0, alignment=[], length0=T, cost0=3.0)
    root.rejpos = -1
    next_beam = [root]
    final_beam = []
    max_batches = T * 2
    tr = dict(tied_pops=0, width_cut_ties=0, cap_cut_ties=0, queue_max=0, finals_max=0, finals_per_pop_max=0, new_keys_max=0,
              rej_inside=0, rej_behind=0, rej_index0=0, rej_raised=0,
              # the rejection rule, per expanded row behind a parent of length > 1: an ordinary parent's misalignment below / not
              # below 0.1; round() met a half and went to the even neighbour below / above; the parent one-hot because the
              # attention gave such a row / because it is a rejection; the source position beyond the line; an eligible row
              # whose source row is all zero
              rej_mis_inside=0, rej_mis_outside=0, half_down=0, half_up=0, is1_by_attention=0, is1_by_rejection=0, beyond_line=0,
              zero_source_row=0,
              # ... and, behind ordinary parents, the largest misalignment below 0.1 and the smallest not below it (None: none met)
              mis_inside_max=None, mis_outside_min=None)
    steps_run = 0
    for l in range(max_batches):
        beam = []
        last = None
        filed = 0
        while next_beam:
            node = next_beam.pop()
            if last is not None and last.pro_cost() == node.pro_cost():
                tr['tied_pops'] += 1
            last = node
            if node.value == '\n':
                insort(final_beam, node)
                filed += 1
            else:
                beam.append(node)
            if len(beam) >= m.batch_size:
                break
        if next_beam and last.pro_cost() == next_beam[-1].pro_cost():
            tr['tied_pops'] += 1                       # (the pop stopped between two equal keys)
        tr['finals_per_pop_max'] = max(tr['finals_per_pop_max'], filed)
        tr['finals_max'] = max(tr['finals_max'], len(final_beam))
        if not beam:
            break
        if len(final_beam) > m.beam_width_out:
            a, b = final_beam[-1].pro_cost(), beam[0].pro_cost()
            if a >= b if 'stop_ge' in rules else a > b:
                break
        steps_run += 1
        target = np.vstack([node.scores for node in beam])
        states_val = [np.vstack([node.state[layer] for node in beam]) for layer in range(len(beam[0].state))]
        scores_output, states_output = m.step(target, attended, states_val, u=u)
        cost_rows = lm_step(m, target, attended, states_val) if lm else None
        made = 0
        for i, node in enumerate(beam):
            states = [layer[i:i + 1] for layer in states_output]
            scores = scores_output[i]
            alignment = states[-1][0]
            misalignment = 0.0
            is1 = False
            if node.length > 1:
                prev_alignment = node.alignment
                prev_source_pos = float(np.matmul(np.asarray(prev_alignment, np.float64), np.arange(T)))
                source_pos = float(np.matmul(alignment.astype(np.float64), np.arange(T)))
                misalignment = abs(source_pos - prev_source_pos - 1)
                is1 = bool(np.max(alignment if 'is1_from_attention_row' in rules else prev_alignment) == 1.0) and 'is1_ignored' not in rules
                if is1:
                    source_pos = int(prev_source_pos) + 1
                    tr['is1_by_rejection' if node.rejpos >= 0 else 'is1_by_attention'] += 1
                else:
                    tr['rej_mis_inside' if misalignment < 0.1 else 'rej_mis_outside'] += 1
                    if misalignment < 0.1:
                        tr['mis_inside_max'] = misalignment if tr['mis_inside_max'] is None else max(tr['mis_inside_max'], misalignment)
                    else:
                        tr['mis_outside_min'] = misalignment if tr['mis_outside_min'] is None else min(tr['mis_outside_min'], misalignment)
                    if source_pos - np.floor(source_pos) == 0.5:
                        tr['half_down' if int(np.floor(source_pos)) % 2 == 0 else 'half_up'] += 1
                    source_pos = int(np.floor(source_pos + 0.5)) if 'round_half_up' in rules else int(round(source_pos))
            else:
                source_pos = 0
            eligible = misalignment < mis_limit or is1 or 'mis_not_tested' in rules
            if source_pos >= T and beyond_line == 'no_candidate':
                tr['beyond_line'] += 1
                source_scores = np.zeros_like(source_seq[0])
            else:
                source_scores = source_seq[source_pos]
                tr['zero_source_row'] += bool(m.rejection_threshold and eligible and not np.any(source_scores))
            if m.rejection_threshold and eligible and np.any(source_scores):
                rej_idx = int(np.nanargmax(source_scores))
                if float(scores[rej_idx]) < m.rejection_threshold:
                    scores[rej_idx] = m.rejection_threshold
                    tr['rej_raised'] += 1
                tr['rej_index0'] += rej_idx == 0
            else:
                rej_idx = None
            if 'tie_low' in rules:
                scores_order = np.argsort(-scores, kind='stable')[::-1]
            else:
                scores_order = np.argsort(scores, kind='stable')
            highest = scores[scores_order[-1]]
            ordered = scores[scores_order].astype(np.float64)
            beampos = V - int(np.searchsorted(ordered, float(highest) * m.beam_threshold_in))
            beampos = min(beampos, m.beam_width_in)
            if 0 < beampos < V and ordered[V - beampos] == ordered[V - beampos - 1]:
                tr['width_cut_ties'] += 1
            pos = 0
            for idx in reversed(scores_order):
                idx = int(idx)
                pos += 1
                score = scores[idx]
                with np.errstate(divide='ignore', invalid='ignore'):
                    logscore = -np.log(cost_rows[i][idx] if lm else score)
                alignment1 = alignment
                rejpos = -1
                if rej_idx is not None and idx == rej_idx:
                    alignment1 = np.eye(T, dtype=alignment.dtype)[source_pos]
                    rejpos = source_pos
                    tr['rej_behind' if pos > beampos else 'rej_inside'] += 1
                    rej_idx = None
                elif pos > beampos:
                    if rej_idx:
                        continue
                    else:
                        break
                value = i_c[idx]
                if np.isnan(logscore) or value == '':
                    continue
                scores1 = np.copy(scores)
                scores[idx] = 0
                child = Node(parent=node, state=states, value=value, scores=scores1, prob=score, cost=logscore, alignment=alignment1)
                child.rejpos = rejpos
                insort(next_beam, child)
                made += 1
        if l + 1 < max_batches:            # (the last iteration's children are never popped: the device does not create them)
            tr['new_keys_max'] = max(tr['new_keys_max'], made)
        tr['queue_max'] = max(tr['queue_max'], len(next_beam))
        cap = max_batches * m.batch_size
        if len(next_beam) > cap:
            if next_beam[-cap].pro_cost() == next_beam[-cap - 1].pro_cost():
                tr['cap_cut_ties'] += 1
            next_beam = next_beam[:cap] if 'cap_other_end' in rules else next_beam[-cap:]
    stats = dict(steps=steps_run, finals=len(final_beam), left=len(next_beam))
    if trace is not None:
        trace.update(tr)
    out = []
    while final_beam:
        node = final_beam.pop()
        nodes = node.to_sequence()[1:]
        out.append((''.join(n.value for n in nodes), [n.prob for n in nodes], node.cum_cost / (node.length - 1),
                    [n.alignment for n in nodes], [n.rejpos for n in nodes]))
    return out, stats


# ------------------------------------------------------------------------------------------------------------------ cases
def _f32(x):
    return float(np.float32(x))


def _ulp(x, n):
    """The float32 n ulps from x (as a Python float)."""
    v = np.float32(x)
    for _ in range(abs(n)):
        v = np.nextafter(v, np.float32(np.inf if n > 0 else -np.inf))
    return float(v)


class Case(object):
    """One search configuration.  lines: lists of vocabulary indices (0 = an unmapped character), each line gets its '\\n';
    shorter lines of a batch are padded (ragged).  family 'uniform' or ('held', group, split01)."""

    def __init__(self, name, family, V, N, lines, width_in=15, threshold_in=0.2, width_out=16, rejection=0.3, lm=False, **promises):
        self.name, self.family, self.V, self.N, self.lines = name, family, V, N, lines
        self.width_in, self.threshold_in, self.width_out, self.rejection, self.lm = width_in, threshold_in, width_out, rejection, lm
        self.promises = promises          # what the CPU test asserts of the oracle's trace / the GPU test of the stats
        self.T = max(len(x) for x in lines) + 1
        self.cfg = ModelConfig(depth=DEPTH, width=WIDTH, voc_size=V)

    @property
    def max_results(self):
        return min(self.width_out + 2, 64)          # casv_decode_beam takes 1..64

    @property
    def form(self):
        return beam_form(self.N, self.V, self.width_in, self.T)

    def weights(self, dtype=np.float32):
        w = uniform_weights(self.cfg) if self.family == 'uniform' else held_weights(self.cfg, *self.family[1:])
        return {k: v.astype(dtype) for k, v in w.items()}

    def model(self, dtype=np.float32):
        return OracleModel(self.cfg, self.weights(dtype), batch_size=self.N, beam_width_in=self.width_in,
                           beam_threshold_in=self.threshold_in, beam_width_out=self.width_out, rejection_threshold=self.rejection)

    def texts(self):
        i_c = make_vocabulary(self.V)[1]
        return [''.join(i_c[v] if v else UNMAPPED for v in line) + '\n' for line in self.lines]

    def inputs(self, m):
        """-> (enc_in (B,T,V) as the reference vectorises the lines, idx (B,T) int32 for casv_encode: -1 = padding)"""
        texts = self.texts()
        enc_in, _, _, _ = vectorize_lines(m, texts, [[] for _ in texts])
        idx = np.where(enc_in.any(axis=2), enc_in.argmax(axis=2), -1).astype(np.int32)
        return enc_in, idx

    def decoder_kwargs(self):
        return dict(batch_size=self.N, beam_width_in=self.width_in, beam_threshold_in=self.threshold_in,
                    beam_width_out=self.width_out, rejection_threshold=self.rejection, max_results=self.max_results)


def run_search(case, dtype=np.float32, rules=(), lm=False):
    """-> per line (results, stats, trace) of `search`."""
    m = case.model(dtype)
    enc_in, _ = case.inputs(m)
    enc = m.encode(enc_in)
    out = []
    for j in range(len(case.lines)):
        trace = {}
        res, stats = search(m, enc_in[j], [e[j:j + 1] for e in enc], rules, trace, lm)
        out.append((res, stats, trace))
    return out


def H(group, split01=True, boost=0.0, emb_scale=4.0):
    return ('held', group, split01, boost, emb_scale)


def _u(V):
    return _f32(np.float32(1) / np.float32(V))


ALL = 1e-4      # a beam_threshold_in below every score ratio of the table: the width alone cuts
CASES = [
    # --- uniform, 4 waves: ln V on both sides of cost0 = 3; beam_width_in 1, 3, 15, 50, >= V; beam_width_out 1, 4, 16, 63
    Case('u_v16_n4', 'uniform', 16, 4, [[5, 9, 3], [7]], width_out=4, cut='width'),
    Case('u_v20_n3', 'uniform', 20, 3, [[5, 9, 3, 4], [7, 2]], width_in=3, threshold_in=ALL, width_out=1, cut='width'),
    Case('u_v24_n1', 'uniform', 24, 1, [[5, 9], [3]], width_in=1, threshold_in=ALL, width_out=1, rejection=0.03, cut='width', behind=True),
    Case('u_v64_n4_lm', 'uniform', 64, 4, [[40, 9, 63], [2, 2]], width_in=50, threshold_in=ALL, width_out=4, lm=True, cut='width'),
    Case('u_v16_all', 'uniform', 16, 4, [[5, 9, 3], [7]], width_in=16, threshold_in=ALL, width_out=16),
    Case('u_v20_all', 'uniform', 20, 8, [[5, 9, 3], [7]], width_in=25, threshold_in=ALL, width_out=63, rejection=0.0),
    # V = 2: only '' and '\n'; unmapped characters (rejection index 0); T = 1 and T = 2; V = 65: the second entry of a lane
    Case('u_v2_n4', 'uniform', 2, 4, [[0, 0], []], width_in=15, width_out=1, rej0=True),
    Case('u_v65_t1', 'uniform', 65, 8, [[]], width_in=1, threshold_in=ALL, width_out=16),
    Case('u_v65_t2', 'uniform', 65, 16, [[64], [0]], width_in=15, threshold_in=ALL, width_out=4, cut='width', rej0=True),
    Case('u_unmapped', 'uniform', 16, 4, [[0, 0, 0], [3, 0]], width_in=15, width_out=4, cut='width', rej0=True),
    # --- rejection threshold at, just above, just below the tied score, 0 and 1.0
    Case('u_rej_eq', 'uniform', 16, 4, [[5, 9, 3]], rejection=_u(16), width_out=4, cut='width'),
    Case('u_rej_above', 'uniform', 16, 4, [[5, 9, 3]], rejection=_ulp(_u(16), 1), width_out=4, cut='width'),
    Case('u_rej_below', 'uniform', 16, 4, [[5, 9, 3]], rejection=_ulp(_u(16), -1), width_out=4, cut='width'),
    Case('u_rej_0', 'uniform', 16, 8, [[5, 9, 3]], rejection=0.0, width_out=4, cut='width'),
    Case('u_rej_1', 'uniform', 24, 8, [[5, 9, 3], [0, 4]], rejection=1.0, width_in=3, threshold_in=ALL, width_out=4, cut='width', rej0=True),
    Case('u_rej_behind', 'uniform', 24, 4, [[2, 3, 2], [0, 2]], rejection=_ulp(_u(24), -1), width_in=3, threshold_in=ALL, width_out=4,
         cut='width', behind=True, rej0=True),
    # --- beam_threshold_in: fl(highest * threshold) exactly a tied score, and one ulp to either side (highest = the rejection's 0.5)
    Case('u_thr_eq', 'uniform', 16, 4, [[5, 9, 3]], rejection=0.5, threshold_in=0.125, width_out=4),
    Case('u_thr_above', 'uniform', 16, 4, [[5, 9, 3]], rejection=0.5, threshold_in=_ulp(0.125, 1), width_out=4),
    Case('u_thr_below', 'uniform', 16, 4, [[5, 9, 3]], rejection=0.5, threshold_in=_ulp(0.125, -1), width_out=4),
    # --- held state: ties inside groups of 4, 2, 8; the source line's characters inside one group
    Case('h4_v24_n4', H(4), 24, 4, [[2, 3, 4], [13, 5]], width_in=3, threshold_in=ALL, width_out=4, cut='width'),
    Case('h4_v64_n8_lm', H(4), 64, 8, [[2, 3, 9, 10], [5]], width_in=15, threshold_in=ALL, width_out=4, lm=True, cut='width'),
    Case('h2_v20_n3', H(2), 20, 3, [[2, 4, 6], [0, 3]], width_in=15, threshold_in=0.05, width_out=1, rej0=True),
    Case('h8_v64_n16', H(8, False), 64, 16, [[2, 3, 4, 5, 6], [9, 17]], width_in=50, threshold_in=0.01, width_out=16),
    Case('h4_thr', H(4), 24, 4, [[2, 3, 4]], width_in=15, threshold_in=0.5, rejection=0.0, width_out=4),
    # --- ending the line is the likeliest child: many finished hypotheses at once (more than pop_cap - N = 64 in one pop: the walk
    #     goes on into the queue in HBM) and more than f_cap = 64 of them in all
    Case('h_finals_n4', H(2, True, 0.5, 0.25), 96, 4, [[5, 9], [7]], width_in=96, threshold_in=ALL, width_out=63),
    Case('h_finals_n16', H(4, True, 0.4, 0.5), 96, 16, [[5, 9], [7]], width_in=96, threshold_in=ALL, width_out=16),
    Case('h_finals_n64_lm', H(2, True, 0.5, 0.25), 200, 64, [[5, 9]], width_in=200, threshold_in=ALL, width_out=63, lm=True, over_f_cap=True,
         staged=False, big_sort=True),
    Case('h_finals_n256', H(2, True, 0.5, 0.25), 96, 256, [[5, 9]], width_in=96, threshold_in=ALL, width_out=63, many_finals=True,
         over_f_cap=True, big_sort=True),
    Case('h_finals_v1100_n256', H(2, True, 0.5, 0.25), 1100, 256, [[5, 9]], width_in=100, threshold_in=ALL, width_out=16, many_finals=True,
         over_f_cap=True, big_sort=True),
    # --- VPL 8, 16, 32, 64 in the 4- and 8-wave forms
    Case('u_v300_n3', 'uniform', 300, 3, [[299, 2]], width_in=15, threshold_in=ALL, width_out=4, cut='width'),
    Case('h4_v300_n8', H(4), 300, 8, [[299, 2]], width_in=15, threshold_in=ALL, width_out=4, cut='width'),
    Case('u_v600_n4', 'uniform', 600, 4, [[599, 2, 300]], width_in=3, threshold_in=ALL, width_out=4, cut='width'),
    Case('h4_v600_n8', H(4), 600, 8, [[599, 2, 300]], width_in=15, threshold_in=ALL, width_out=4),
    Case('u_v1100_n4', 'uniform', 1100, 4, [[1099, 2]], width_in=3, threshold_in=ALL, width_out=4, cut='width'),
    Case('h4_v1100_n64', H(4), 1100, 64, [[1099, 2]], width_in=50, threshold_in=ALL, width_out=4, staged=False),
    Case('u_v2100_n1', 'uniform', 2100, 1, [[2099, 64]], width_in=15, threshold_in=ALL, width_out=1, cut='width'),
    Case('h8_v2100_n8', H(8, False), 2100, 8, [[2099, 2]], width_in=15, threshold_in=ALL, width_out=4),
    Case('u_v4096_n16', 'uniform', 4096, 16, [[4095, 2]], width_in=3, threshold_in=ALL, width_out=4, cut='width'),
    # --- the queue reaches 2*T*N and is cut inside a tie group
    Case('u_cap_n4', 'uniform', 64, 4, [[5, 9], [7]], width_in=50, threshold_in=0.01, width_out=63, rejection=0.0, cut='cap'),
    Case('u_cap_n8', 'uniform', 20, 8, [[5, 9, 3, 4], [7]], width_in=15, threshold_in=ALL, width_out=16, cut='cap'),
    # --- 16 waves, phase A as a grid of its own; queue in HBM; new keys beyond the sort capacity
    Case('u_v24_n64', 'uniform', 24, 64, [[5, 9, 3], [7]], width_in=15, threshold_in=ALL, width_out=16, cut='width', staged=True, big_sort=False),
    Case('u_cap_n64', 'uniform', 64, 64, [[5, 9, 3], [7]], width_in=50, threshold_in=ALL, width_out=16, cut='cap', big_sort=False,
         staged=False),
    Case('h4_v200_n256_lm', H(4), 200, 256, [[2, 3, 9], [5]], width_in=3, threshold_in=ALL, width_out=16, lm=True, cut='width'),
    Case('u_v512_n64', 'uniform', 512, 64, [[500, 2]], width_in=15, threshold_in=ALL, width_out=4, cut='width'),
    Case('h4_v1000_n64', H(4), 1000, 64, [[999, 2]], width_in=15, threshold_in=ALL, width_out=4),
    Case('u_v1024_n256', 'uniform', 1024, 256, [[999, 2]], width_in=3, threshold_in=ALL, width_out=4, cut='width'),
    Case('u_v96_n256_big', 'uniform', 96, 256, [[5, 9], [7]], width_in=50, threshold_in=0.01, width_out=63, rejection=0.1, big_sort=True,
         cut='cap', staged=True),
    Case('h4_v96_n256_big', H(4), 96, 256, [[5, 9, 6]], width_in=50, threshold_in=ALL, width_out=16, big_sort=True, staged=False),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ------------------------------------------------------------------------------------------------------------------ device results
# What the GPU tests of the tables (tests/test_gpu_beam_ties.py, tests/test_gpu_steered_attention.py) share: results of
# casv_decode_beam cut to their lengths, against each other bit for bit and against `search`.
RT, AT = 2e-4, 2e-6


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same_bits(a, b, what):
    assert len(a) == len(b)
    for j, (x, y) in enumerate(zip(a, b)):
        assert (x['n_found'], x['n_steps'], len(x['results'])) == (y['n_found'], y['n_steps'], len(y['results'])), (what, j)
        for k, (p, q) in enumerate(zip(x['results'], y['results'])):
            for key in ('idx', 'rej', 'lo'):
                assert np.array_equal(p[key], q[key]), (what, j, k, key)
            for key in ('prob', 'align', 'w'):
                assert np.array_equal(bits(p[key]), bits(q[key])), (what, j, k, key)
            assert p['score'].view(np.int64) == q['score'].view(np.int64), (what, j, k)


def against_the_oracle(case, got, want, c_i):
    T, V = case.T, case.V
    exact = {int(bits(np.float32(1) / np.float32(V)))}
    if case.rejection:
        exact.add(int(bits(np.float32(case.rejection))))
    for j, (dev, (res, stats, rej, _)) in enumerate(zip(got, want)):
        assert dev['n_found'] == stats['finals'] and dev['n_steps'] == stats['steps'], (j, dev['n_found'], dev['n_steps'], stats)
        assert len(dev['results']) == min(len(res), case.max_results), j
        assert not dev['empty'].any(), j
        for k, d in enumerate(dev['results']):
            text, probs, score, aligns = res[k][:4]
            where = (case.name, j, k, text)
            assert list(d['idx']) == [c_i[ch] for ch in text], where
            assert list(d['rej']) == rej[k], where
            p = np.asarray(probs, np.float32)
            pinned = np.isin(bits(p), list(exact))
            assert np.array_equal(bits(d['prob'])[pinned], bits(p)[pinned]), where
            assert np.allclose(d['prob'], p, rtol=RT, atol=0), where
            assert abs(d['score'] - score) <= RT * abs(score), where
            a = np.asarray(aligns, np.float32).reshape(len(text), T)
            assert np.allclose(d['align'], a, rtol=RT, atol=AT), where
            window = np.zeros_like(d['align'])
            for s in range(len(text)):
                if rej[k][s] >= 0:
                    assert np.array_equal(d['align'][s], np.eye(T, dtype=np.float32)[rej[k][s]]), where
                    assert d['lo'][s] == rej[k][s] and d['w'][s, 0] == 1 and not d['w'][s, 1:].any(), where
                assert d['lo'][s] >= 0, where
                n = min(d['w'].shape[1], T - int(d['lo'][s]))
                window[s, d['lo'][s]:d['lo'][s] + n] = d['w'][s, :n]
                assert not d['w'][s, n:].any(), where
            assert np.array_equal(bits(window), bits(d['align'])), where
