"""lm_predict restated on top of the oracle -- test infrastructure (the package `oracle/` stays as it is).

The reference's decoder can run as a context-free character language model (seq2seq.py:145-149, 419-473): the top (attention)
layer once more on the decoder's own top-layer input and states, with zero attention constants, through the tied projection.
Its beam search then rates every child by the LM (seq2seq.py:1487-1490) and keeps choosing the children by the decoder's scores.

``lm_step``                  <- seq2seq.py:464-470 (the LM output of decoder_model)
``decode_sequence_beam_lm``  <- oracle/decode.py decode_sequence_beam with the one-line cost change of seq2seq.py:1487-1490
"""
from bisect import insort_left

import numpy as np

from oracle.decode import Node
from oracle.model import decoder_step


def lm_step(m, p_in, enc_out, states, window_dtype=None):
    """LM probabilities (R,V) of one decoder_model call: oracle.model.decoder_step with enc_out AND u set to zeros
    (`constants=[attention_zero, attention_zero]`, s2s:466-470).  The lower layers are the decoder's own; the attention has one
    energy at every position of the window, so the context is exactly 0 -- or NaN where the window is empty or the energy is 0 or
    infinite.  The LM cell's states are discarded.  window_dtype: oracle.model.attention."""
    dt = m.weights['E'].dtype
    z = np.zeros(np.asarray(enc_out).shape, dt)
    u = np.zeros(z.shape[:2] + (m.cfg.width,), dt)
    p, _ = decoder_step(m.cfg, m.weights, p_in, z, states, u=u, window_dtype=window_dtype)
    return p


def decode_sequence_beam_lm(m, source_seq=None, encoder_outputs=None, stats=None):
    """decode_sequence_beam (oracle/decode.py) with lm_predict: a child's cost is -log of the LM's probability of its index, and
    a NaN LM probability drops the child.  Yields (text, probs, cum_cost/(length-1), alignments, rejection positions) best first;
    rejection position = the source position of a rejection step (one-hot alignment, s2s:1495), else -1."""
    V = m.voc_size
    i_c = m.mapping[1]
    if encoder_outputs is None:
        encoder_outputs = m.encode(np.expand_dims(source_seq, axis=0))
    attended = encoder_outputs[0]
    T = attended.shape[1]
    u = None if m.recompute_u else attended @ m.weights['att_U']
    states_values = list(encoder_outputs[1:])
    next_beam = [Node(state=states_values, value='', scores=np.zeros(V), prob=[], cost=0.0,
                      alignment=[], length0=T, cost0=3.0)]
    next_beam[0].rejpos = -1
    final_beam = []
    max_batches = T * 2
    steps_run = 0
    for l in range(max_batches):
        beam = []
        while next_beam:
            node = next_beam.pop()
            if node.value == '\n':
                insort_left(final_beam, node)
            else:
                beam.append(node)
            if len(beam) >= m.batch_size:
                break
        if not beam:
            break
        if (len(final_beam) > m.beam_width_out and
                final_beam[-1].pro_cost() > beam[0].pro_cost()):
            break
        steps_run += 1
        target = np.vstack([node.scores for node in beam])
        states_val = [np.vstack([node.state[layer] for node in beam])
                      for layer in range(len(beam[0].state))]
        scores_output, states_output = m.step(target, attended, states_val, u=u)
        lmscores_output = lm_step(m, target, attended, states_val)          # s2s:1431-1433
        for i, node in enumerate(beam):
            states = [layer[i:i + 1] for layer in states_output]
            scores = scores_output[i]
            alignment = states[-1][0]
            misalignment = 0.0
            if node.length > 1:
                prev_alignment = node.alignment
                prev_source_pos = float(np.matmul(np.asarray(prev_alignment, np.float64), np.arange(T)))
                source_pos = float(np.matmul(alignment.astype(np.float64), np.arange(T)))
                misalignment = abs(source_pos - prev_source_pos - 1)
                if np.max(prev_alignment) == 1.0:
                    source_pos = int(prev_source_pos) + 1
                else:
                    source_pos = int(round(source_pos))
            else:
                source_pos = 0
            source_scores = source_seq[source_pos]
            if (m.rejection_threshold
                    and (misalignment < 0.1 or (len(node.alignment) and np.max(node.alignment) == 1.0))
                    and np.any(source_scores)):
                rej_idx = int(np.nanargmax(source_scores))
                if float(scores[rej_idx]) < m.rejection_threshold:
                    scores[rej_idx] = m.rejection_threshold
            else:
                rej_idx = None
            scores_order = np.argsort(scores, kind='stable')
            highest = scores[scores_order[-1]]
            beampos = V - int(np.searchsorted(scores[scores_order].astype(np.float64),
                                              float(highest) * m.beam_threshold_in))
            beampos = min(beampos, m.beam_width_in)
            pos = 0
            for idx in reversed(scores_order):
                idx = int(idx)
                pos += 1
                score = scores[idx]
                with np.errstate(divide='ignore', invalid='ignore'):
                    logscore = -np.log(lmscores_output[i][idx])      # s2s:1487-1490: the LM rates the child
                alignment1 = alignment
                rejpos = -1
                if rej_idx is not None and idx == rej_idx:
                    alignment1 = np.eye(T, dtype=alignment.dtype)[source_pos]
                    rejpos = source_pos
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
                child = Node(parent=node, state=states, value=value, scores=scores1,
                             prob=score, cost=logscore, alignment=alignment1)
                child.rejpos = rejpos
                insort_left(next_beam, child)
        if len(next_beam) > max_batches * m.batch_size:
            next_beam = next_beam[-max_batches * m.batch_size:]
    if stats is not None:
        stats['steps'] = steps_run
        stats['finals'] = len(final_beam)
        stats['left'] = len(next_beam)
    while final_beam:
        node = final_beam.pop()
        nodes = node.to_sequence()[1:]
        yield (''.join(n.value for n in nodes),
               [n.prob for n in nodes],
               node.cum_cost / (node.length - 1),
               [n.alignment for n in nodes],
               [n.rejpos for n in nodes])
