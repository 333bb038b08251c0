"""Host side of `Sequence2Sequence.train()` (seq2seq.py:590-649 + lib/keras_train.py:27-438): epochs over the
generator, validation, early stopping / NaN termination / per-epoch checkpoints.  Each batch is ONE call into
the C ABI (`casv_train_step`), which runs forward, backward, clipping and Adam on the device.  With a teacher
(distillation) a batch is the teacher's scoring call, its K alternatives per position and `casv_train_step_soft`; with a
sample schedule (scheduled sampling) it is `casv_train_step_sampled` at the epoch's ratio; with risk samples (minimum-risk
training) it is slices of sources with their candidate sets, each `casv_train_step_risk` (`risk_step`)."""
import math
import queue
import signal
import threading

import numpy as np

from . import keras_h5


def prefetch(iterable, depth=2, cancel=None, in_call=None, detach_after=None):
    """Run `iterable` in a worker thread, `depth` items ahead of the consumer -- the reference feeds `train_on_batch` from a
    `GeneratorEnqueuer` worker (keras_train.py:133-145) so that vectorising the next batch overlaps the device step; here the
    C ABI call releases the GIL for the whole step, so a thread does.  Exceptions of the producer surface in the consumer;
    a consumer that stops early (NaN loss, stop signal) releases the producer.

    Leaving early: the worker is joined, however long its current `next(iterable)` takes (the default: train()'s producers draw
    from the model's random generator and read its state -- a worker left behind would keep doing so beside whatever the caller
    does next).  Stages whose producer may block for good on something outside this process (correct_batches: a user generator
    reading a pipe, a nested stage) pass `detach_after`: such a worker is left behind after that many seconds (a daemon thread; its
    next put() sees `stop`) -- except while `in_call` (an Event the producer sets around its C-ABI calls) is set: the caller must
    not get the engine back while a call runs on it, the handle is not thread-safe.  `cancel`: an Event of the caller that ends
    the consumer loop as well (a nested stage's consumer is another stage's worker: it must not sit in q.get() for good)."""
    q = queue.Queue(maxsize=max(1, depth))
    done, stop = object(), threading.Event()

    def put(item):
        while not stop.is_set():
            try:
                q.put(item, timeout=0.1)
                return True
            except queue.Full:
                continue
        return False

    def work():
        try:
            for item in iterable:
                if not put(('item', item)):
                    return
        except BaseException as err:            # handed to the consumer
            put(('error', err))
            return
        put(('done', done))

    thread = threading.Thread(target=work, name='casv-batch-prefetch', daemon=True)
    thread.start()
    try:
        while True:
            if cancel is None:
                kind, item = q.get()
            else:
                try:
                    kind, item = q.get(timeout=0.1)
                except queue.Empty:
                    if cancel.is_set():
                        return
                    continue
            if kind == 'done':
                return
            if kind == 'error':
                raise item
            yield item
    finally:
        stop.set()
        waited = 0.0
        while thread.is_alive():
            thread.join(0.1)
            if in_call is not None and in_call.is_set():
                continue                        # a device call of the worker is in flight: wait it out, however long it takes
            waited += 0.1
            if detach_after is not None and waited >= detach_after:
                break


def train_batches(s2s, filenames, split_rand, rng):
    """One epoch of training batches in the form `casv_train_step` takes: index arrays of vectorize_lines, the random
    degradation of seq2seq.py:909-915, the dropout keep-masks (drawn in this order per batch)."""
    for batch in s2s.gen_lines(filenames, True, split_rand, True):
        if not batch:
            return                                 # end of epoch (kt:160-162)
        src, conf, tgt, _ = batch
        idx, val, dec_in, dec_out, w = batch_to_indices(s2s, src, tgt, conf)
        idx, val = degrade(idx, val, rng)
        yield idx, val, dec_in, dec_out, w, dropout_masks(s2s, len(src), rng)


def validation_batches(s2s, filenames, split_rand):
    for batch in s2s.gen_lines(filenames, True, split_rand, False):
        if not batch:
            return
        src, conf, tgt, _ = batch
        yield batch_to_indices(s2s, src, tgt, conf)


def line_batches(s2s, filenames, split_rand):
    """One epoch of training batches as gen_lines loads them, (source lines, confidences, target lines): what `risk_step` takes."""
    for batch in s2s.gen_lines(filenames, True, split_rand, True):
        if not batch:
            return
        src, conf, tgt, _ = batch
        yield src, conf, tgt


def batch_to_indices(s2s, lines_source, lines_target, lines_conf):
    """The arrays of vectorize_lines (seq2seq.py:1020-1119) in index form: encoder (idx, val) (B,T,A),
    decoder input / target character indices (B,U) with -1 for true-zero rows, temporal weights (B,U)."""
    idx, val, _ = s2s._sparse_lines(lines_source, lines_conf)
    return (idx, val) + targets_to_indices(s2s, lines_target)


def targets_to_indices(s2s, lines_target):
    """The decoder side of batch_to_indices: (dec_in, dec_out, weights), each (B,U)."""
    B = len(lines_target)
    U = max(map(len, lines_target)) + 1
    dec_in = np.full((B, U), -1, np.int32)
    dec_out = np.full((B, U), -1, np.int32)
    for i, line in enumerate(lines_target):
        codes = [s2s._index(c, 'decoder input', i) for c in line]
        dec_in[i, 1:len(codes) + 1] = codes
        dec_out[i, :len(codes)] = codes
    weights = (dec_out >= 0).astype(np.float32)
    return dec_in, dec_out, weights


def degrade(idx, val, rng):
    """Random degradation of one encoder position per line to index 0 for learning underspecification
    (seq2seq.py:909-915): position = int(T * U(0,1) / 0.01), applied when it falls inside the line."""
    B, T = idx.shape[:2]
    pos = (T * rng.uniform(0, 1, B) / 0.01).astype(int)
    for b in np.nonzero(pos < T)[0]:
        idx[b, pos[b], :] = -1
        idx[b, pos[b], 0] = 0
        val[b, pos[b], :] = 0
        val[b, pos[b], 0] = 1
    return idx, val


def dropout_masks(s2s, B, rng):
    """Keep-masks of the reference's dropout layers, scaled by 1/(1-rate): time-constant feature masks after
    every encoder layer and every hidden decoder layer (noise_shape (1, F), seq2seq.py:293-298,363-367), a
    per-sample mask on the attention cell's input (LSTMCell(dropout), seq2seq.py:345)."""
    rate = float(s2s.dropout or 0.0)
    if rate <= 0.0:
        return None
    W, d = s2s.width, s2s.depth
    deep = bool(getattr(s2s, 'deep_bidirectional_encoder', False))      # every encoder layer 2W wide (seq2seq.py:292-295)
    C = 2 * W if (d == 1 or deep) else W
    keep = lambda shape: ((rng.uniform(0, 1, shape) >= rate) / (1.0 - rate)).astype(np.float32)
    return {'enc': [keep(2 * W if (n == 0 or deep) else W) for n in range(d)], 'dec': [keep(W) for _ in range(d - 1)],
            'cell': keep((B, W + C))}


ADAM = (1e-3, 0.9, 0.999, 1e-7, 5.0)        # Adam(clipnorm=5) with Keras defaults (seq2seq.py:496), HipEngine.train_begin's


def resume_state(s2s, filename):
    """The training state of checkpoint `filename`, checked against the model: width, depth, mapping, topology flags and frozen
    set must be those of `s2s`.  Raises ValueError with the first difference."""
    state = keras_h5.read_training_state(filename)
    if state is None:
        raise ValueError('cannot resume from "%s": it holds weights only (write checkpoints with checkpoint_training_state = True)'
                         % filename)
    config = keras_h5.read_config(filename)
    mine = s2s._config_dict()
    for key, value in mine.items():
        if key not in config:
            raise ValueError('cannot resume from "%s": its config has no "%s"' % (filename, key))
        theirs = np.asarray(config[key])
        if theirs.shape != np.asarray(value).shape or not np.array_equal(theirs, np.asarray(value)):
            raise ValueError('cannot resume from "%s": %s differs (file %s, model %s)' % (filename, key, theirs.tolist(),
                                                                                          np.asarray(value).tolist()))
    if sorted(state['frozen']) != sorted(s2s.frozen_prefixes):
        raise ValueError('cannot resume from "%s": frozen layers differ (file %s, model %s)' % (filename, state['frozen'],
                                                                                                list(s2s.frozen_prefixes)))
    return state


def check_teacher(s2s, teacher, distill_k, distill_alpha):
    """What distillation asks of the pair, checked on the host before anything runs: the teacher is another, loaded model with the
    student's vocabulary size and character mapping (the soft targets are the teacher's indices), K + 1 slots fit the loss head,
    alpha is a share.  Raises ValueError with the first difference."""
    if teacher is s2s:
        raise ValueError('cannot distil a model from itself')
    if getattr(teacher, 'status', 0) != 2:
        raise ValueError('the teacher must be a configured and loaded model (status 2), its status is %r' % getattr(teacher, 'status', None))
    if teacher.voc_size != s2s.voc_size:
        raise ValueError('teacher and student differ in voc_size (teacher %d, student %d)' % (teacher.voc_size, s2s.voc_size))
    if teacher.mapping[0] != s2s.mapping[0]:
        theirs, mine = teacher.mapping[0], s2s.mapping[0]
        char = next(c for c in sorted(set(theirs) | set(mine)) if theirs.get(c) != mine.get(c))
        raise ValueError('teacher and student differ in their character mapping (%r: teacher %r, student %r)'
                         % (char, theirs.get(char), mine.get(char)))
    most = min(s2s.voc_size, 64) - 1
    if int(distill_k) != distill_k or not 1 <= distill_k <= most:
        raise ValueError('distill_k must be in [1, min(voc_size, 64) - 1] = [1, %d], got %r' % (most, distill_k))
    if not 0.0 <= float(distill_alpha) <= 1.0:
        raise ValueError('distill_alpha must be in [0, 1], got %r' % (distill_alpha,))


def check_distill_resume(state, filename, teacher, distill_k, distill_alpha):
    """A distilled run resumes as a distilled run with the same K and alpha, a plain run as a plain run: ValueError otherwise."""
    theirs = state.get('distill')
    if theirs is None and teacher is None:
        return
    if theirs is None:
        raise ValueError('cannot resume from "%s": it was trained without a teacher' % filename)
    if teacher is None:
        raise ValueError('cannot resume from "%s": it was distilled (distill_k %d, distill_alpha %r), the teacher is missing'
                         % (filename, theirs[0], theirs[1]))
    if (int(theirs[0]), float(theirs[1])) != (int(distill_k), float(distill_alpha)):
        raise ValueError('cannot resume from "%s": distillation differs (file distill_k %d, distill_alpha %r; now %d, %r)'
                         % (filename, theirs[0], theirs[1], distill_k, distill_alpha))


def distill_step(engine, teacher_engine, batch, distill_k, distill_alpha):
    """One training batch with a teacher: the teacher scores the batch as the student sees it, its K likeliest characters per
    position become the soft targets, the student takes the soft step."""
    from .seq2seq import alternatives_to_soft_targets
    idx, val, dec_in, dec_out, w, masks = batch
    teacher_engine.score_targets(idx, val, dec_in, dec_out)
    alt_idx, alt_logp, _ = teacher_engine.score_alternatives(distill_k, want_entropy=False)
    soft_idx, soft_q = alternatives_to_soft_targets(alt_idx, alt_logp, dec_out, alpha=distill_alpha)
    return engine.train_step_soft(idx, val, dec_in, soft_idx, soft_q, w, masks, mode=1)


SCHEDULES = ('linear', 'sigmoid', 'exponential')


def schedule_name(sample_schedule):
    """What a checkpoint records of `sample_schedule`: the name, 'const:<ratio>' of a float, 'callable' of a callable."""
    if callable(sample_schedule):
        return 'callable'
    if isinstance(sample_schedule, str):
        return sample_schedule
    return 'const:%r' % float(sample_schedule)


def schedule_ratio(sample_schedule, epoch, epochs):
    """The sampling ratio of the epoch that follows `epoch` completed ones, out of `epochs`.  The named schedules are the
    reference's formulas at attenuation 3 (seq2seq.py:867-873), which it evaluates at the end of every epoch for the next one
    and starts from 0: linear 3 (epoch - 1) / (epochs - 1), clamped to [0, 1] and 0 where epochs == 1; sigmoid
    1 / (1 + exp(5 - 30 epoch / epochs)); exponential 1 - 0.9 ** (150 epoch / epochs).  A float is that ratio in every epoch; a
    callable is asked with `epoch`.  Raises ValueError for a ratio outside [0, 1]."""
    attenuation = 3
    if callable(sample_schedule):
        ratio = float(sample_schedule(epoch))
    elif not isinstance(sample_schedule, str):
        ratio = float(sample_schedule)
    elif epoch < 1:
        ratio = 0.0
    elif sample_schedule == 'linear':
        ratio = 0.0 if epochs <= 1 else min(1.0, max(0.0, attenuation * (epoch - 1) / (epochs - 1)))
    elif sample_schedule == 'sigmoid':
        ratio = 1 / (1 + math.exp(5 - 10 * attenuation * epoch / epochs))
    else:
        ratio = 1 - 0.9 ** (50 * attenuation * epoch / epochs)
    if not 0.0 <= ratio <= 1.0:             # (NaN fails too)
        raise ValueError('sample_schedule gives the ratio %r for epoch %d: it must lie in [0, 1]' % (ratio, epoch))
    return ratio


def cut_is_set(top_k, top_p):
    """Whether (top_k, top_p) truncates anything: (0, 1.0) is no cut."""
    return int(top_k) != 0 or float(top_p) != 1.0


def check_cut(top_k, top_p, what=''):
    """A cut's rules (casv_sample_cut): top_k an int in [0, 4095], top_p in (0, 1].  ValueError with the first fault."""
    try:
        ok = int(top_k) == top_k and 0 <= int(top_k) <= 4095
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError('%stop_k must be an int in [0, 4095] (0: none), got %r' % (what, top_k))
    try:
        ok = 0.0 < float(top_p) <= 1.0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError('%stop_p must lie in (0, 1] (1: none), got %r' % (what, top_p))


def check_sampling(sample_schedule, sample_pick, sample_passes, sample_temperature, teacher, sample_top_k=0, sample_top_p=1.0):
    """The scheduled-sampling keywords of train(), checked on the host before anything runs: ValueError with the first fault."""
    if teacher is not None:
        raise ValueError('sample_schedule together with teacher: soft targets and scheduled sampling do not combine')
    if isinstance(sample_schedule, str):
        if sample_schedule not in SCHEDULES:
            raise ValueError('sample_schedule must be one of %s, a float or a callable, got %r' % (', '.join(SCHEDULES), sample_schedule))
    elif not callable(sample_schedule):
        try:
            ok = 0.0 <= float(sample_schedule) <= 1.0
        except (TypeError, ValueError):
            raise ValueError('sample_schedule must be one of %s, a float or a callable, got %r' % (', '.join(SCHEDULES), sample_schedule))
        if not ok:
            raise ValueError('sample_schedule as a float is a ratio in [0, 1], got %r' % (sample_schedule,))
    if sample_pick not in ('greedy', 'sample'):
        raise ValueError("sample_pick must be 'greedy' or 'sample', got %r" % (sample_pick,))
    if int(sample_passes) != sample_passes or not 1 <= sample_passes <= 8:
        raise ValueError('sample_passes must be in [1, 8], got %r' % (sample_passes,))
    if not (math.isfinite(float(sample_temperature)) and float(sample_temperature) > 0.0):
        raise ValueError('sample_temperature must be finite and positive, got %r' % (sample_temperature,))
    check_cut(sample_top_k, sample_top_p, 'sample_')
    if sample_pick == 'greedy' and cut_is_set(sample_top_k, sample_top_p):
        raise ValueError("sample_top_k / sample_top_p truncate the 'sample' pick: they do not combine with sample_pick='greedy'")


def check_sampling_resume(state, filename, settings):
    """A scheduled-sampling run resumes with the settings it recorded (its seed is taken from the file), a plain run as a
    plain run: ValueError otherwise."""
    theirs = state.get('sample')
    if theirs is None and settings is None:
        return
    if theirs is None:
        raise ValueError('cannot resume from "%s": it was trained without a sample schedule' % filename)
    if settings is None:
        raise ValueError('cannot resume from "%s": it was trained with the sample schedule %r' % (filename, theirs['schedule']))
    for key in ('schedule', 'pick', 'passes', 'temperature', 'top_k', 'top_p'):       # (the cut is recorded only where one is set)
        if theirs.get(key) != settings.get(key):
            raise ValueError('cannot resume from "%s": sample %s differs (file %r, now %r)' % (filename, key, theirs.get(key), settings.get(key)))


def check_risk(s2s, risk_samples, risk_alpha, risk_temperature, risk_top_k, risk_top_p, proposal, teacher, sample_schedule):
    """The minimum-risk keywords of train(), checked on the host before anything runs: ValueError with the first fault.  The
    proposal (None: a private copy of the model) is checked like a teacher: another, loaded model with this model's vocabulary
    size and character mapping -- its candidates are vectorised with this model's mapping."""
    if teacher is not None:
        raise ValueError('risk_samples together with teacher: soft targets and minimum-risk training do not combine')
    if sample_schedule is not None:
        raise ValueError('risk_samples together with sample_schedule: scheduled sampling and minimum-risk training do not combine')
    try:
        ok = int(risk_samples) == risk_samples and 2 <= int(risk_samples) <= 64
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError('risk_samples must be an int in [2, 64] (0: none), got %r' % (risk_samples,))
    if risk_samples > s2s.batch_size:
        raise ValueError('risk_samples=%d candidates per source do not fit batch_size=%d decoder rows' % (risk_samples, s2s.batch_size))
    for name, value in (('risk_alpha', risk_alpha), ('risk_temperature', risk_temperature)):
        try:
            ok = math.isfinite(float(value)) and float(value) > 0.0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError('%s must be finite and positive, got %r' % (name, value))
    check_cut(risk_top_k, risk_top_p, 'risk_')
    if proposal is None:
        return
    if proposal is s2s:
        raise ValueError('the proposal must be another model than the one in training (None: a private copy of it)')
    if getattr(proposal, 'status', 0) != 2:
        raise ValueError('the proposal must be a configured and loaded model (status 2), its status is %r' % getattr(proposal, 'status', None))
    if proposal.voc_size != s2s.voc_size:
        raise ValueError('proposal and model differ in voc_size (proposal %d, model %d)' % (proposal.voc_size, s2s.voc_size))
    if proposal.mapping[0] != s2s.mapping[0]:
        theirs, mine = proposal.mapping[0], s2s.mapping[0]
        char = next(c for c in sorted(set(theirs) | set(mine)) if theirs.get(c) != mine.get(c))
        raise ValueError('proposal and model differ in their character mapping (%r: proposal %r, model %r)'
                         % (char, theirs.get(char), mine.get(char)))


def check_risk_resume(state, filename, settings):
    """A minimum-risk run resumes with the settings it recorded (its seed is taken from the file), a plain run as a plain run:
    ValueError otherwise."""
    theirs = state.get('risk')
    if theirs is None and settings is None:
        return
    if theirs is None:
        raise ValueError('cannot resume from "%s": it was trained without risk_samples' % filename)
    if settings is None:
        raise ValueError('cannot resume from "%s": it was trained with risk_samples=%r' % (filename, theirs['samples']))
    for key in ('samples', 'alpha', 'temperature', 'top_k', 'top_p', 'own_proposal', 'costs'):
        if theirs.get(key) != settings.get(key):
            raise ValueError('cannot resume from "%s": risk %s differs (file %r, now %r)' % (filename, key, theirs.get(key), settings.get(key)))


def proposal_copy(s2s):
    """A second model of `s2s`'s shape, mapping and device with a handle of its own, for the candidates of a minimum-risk run
    without a given proposal; train_files installs the training weights at the start of every epoch."""
    copy = type(s2s)(logger=s2s.logger, progbars=False, device=s2s.device)
    for name in ('batch_size', 'stateful', 'width', 'depth', 'residual_connections', 'deep_bidirectional_encoder', 'bridge_dense',
                 'arithmetic', 'voc_size'):
        setattr(copy, name, getattr(s2s, name))
    copy.mapping = s2s.mapping
    copy._rng = np.random.default_rng(0)     # (configure()'s initial weights are replaced before use: nothing is drawn from the model's generator)
    copy.configure()
    copy.status = 2
    return copy


def risk_candidates(proposal, src, conf, tgt, settings, first_stream):
    """The candidate sets of the sources `src`: per source the gold line `tgt` as candidate 0 and samples - 1 lines drawn from the
    proposal (stream ids first_stream + the source's index).  Returns (candidates, cost): the lists per source and the float32
    costs in row order g * samples + i -- the candidate's edit distance to the gold line over max(len(gold), 1), and -1 for an
    exact duplicate of an earlier candidate of the same source (not a member of its set).  The distances are one row of the
    N x N matrix that `consensus_of` computes on the device; with settings['edit_costs'] (an `EditCosts`) it is the distance under
    those costs over unit x max(len(gold), 1).  A duplicate is an equal string, whatever the costs."""
    n = settings['samples']
    drawn = proposal.sample_lines(src, conf, n=n - 1, temperature=settings['temperature'], top_k=settings['top_k'], seed=settings['seed'],
                                  streams=[first_stream + j for j in range(len(src))], top_p=settings['top_p'])[0]
    candidates = [[gold] + list(lines) for gold, lines in zip(tgt, drawn)]
    costs = settings.get('edit_costs')       # (the EditCosts of a run with risk_costs; its recorded form is settings['costs'])
    unit = 1 if costs is None else costs.unit
    dists = proposal.consensus_of(candidates, distances=True, **({} if costs is None else {'costs': costs}))[2]
    cost = np.empty((len(src) * n,), np.float32)
    for g, cands in enumerate(candidates):
        assert len(cands) == n, 'source %d has %d candidates, not %d' % (g, len(cands), n)
        for i, line in enumerate(cands):
            cost[g * n + i] = -1.0 if line in cands[:i] else dists[g][0][i] / (unit * max(len(cands[0]), 1))
    return candidates, cost


def risk_step(engine, proposal, batch, settings, rng):
    """One loaded training batch (source lines, confidences, target lines) under minimum-risk training: the batch is taken
    batch_size // samples sources at a time, so that a step never has more decoder rows than batch_size; each slice gets its
    candidate sets (`risk_candidates`), is vectorised as a hard batch would be -- the sources degraded and repeated once per
    candidate, the dropout masks drawn for the slice's rows -- and stepped with `HipEngine.train_step_risk`.  settings: the run's
    recorded settings plus 'model' (whose mapping vectorises), 'batch_size' and 'stream', the running number of the next line,
    which this advances.  Returns the slices' losses."""
    s2s, n = settings['model'], settings['samples']
    src, conf, tgt = batch
    per_slice = max(settings['batch_size'] // n, 1)
    losses = []
    for start in range(0, len(src), per_slice):
        part = slice(start, start + per_slice)
        lines, lines_conf = src[part], (conf[part] if conf else conf)
        candidates, cost = risk_candidates(proposal, lines, lines_conf, tgt[part], settings, settings['stream'])
        settings['stream'] += len(lines)
        idx, val, _ = s2s._sparse_lines(lines, lines_conf)
        idx, val = degrade(idx, val, rng)
        idx, val = np.repeat(idx, n, axis=0), np.repeat(val, n, axis=0)
        dec_in, dec_out, w = targets_to_indices(s2s, [line for cands in candidates for line in cands])
        masks = dropout_masks(s2s, len(lines) * n, rng)
        loss, _ = engine.train_step_risk(idx, val, dec_in, dec_out, w, cost, n, settings['alpha'], masks, mode=1)
        losses.append(loss)
        if not np.isfinite(loss):
            break
    return losses


def train_files(s2s, filenames, val_filenames=None, resume=None, teacher=None, distill_k=8, distill_alpha=0.5,
                sample_schedule=None, sample_pick='greedy', sample_passes=1, sample_temperature=1.0, sample_top_k=0, sample_top_p=1.0,
                risk_samples=0, risk_alpha=1.0, risk_temperature=1.0, risk_top_k=0, risk_top_p=1.0, proposal=None, risk_costs=None):
    risk = None                              # minimum-risk training: what the checkpoints record (the seed joins below)
    if risk_samples:
        check_risk(s2s, risk_samples, risk_alpha, risk_temperature, risk_top_k, risk_top_p, None, teacher, sample_schedule)
        risk = {'samples': int(risk_samples), 'alpha': float(risk_alpha), 'temperature': float(risk_temperature),
                'top_k': int(risk_top_k), 'top_p': float(risk_top_p), 'own_proposal': proposal is None}
        if risk_costs is not None:           # (only where set: a run without costs writes the checkpoints it always wrote)
            if not hasattr(risk_costs, 'settings'):
                raise ValueError('risk_costs=%r: None or an EditCosts' % (risk_costs,))
            risk['costs'] = risk_costs.settings()
    elif proposal is not None:
        raise ValueError('proposal without risk_samples: there is nothing to propose for')
    elif risk_costs is not None:
        raise ValueError('risk_costs without risk_samples: there is no candidate to cost')
    sampling = None                          # scheduled sampling: what the checkpoints record (the seed joins below)
    if sample_schedule is not None:
        check_sampling(sample_schedule, sample_pick, sample_passes, sample_temperature, teacher, sample_top_k, sample_top_p)
        sampling = {'schedule': schedule_name(sample_schedule), 'pick': sample_pick, 'passes': int(sample_passes),
                    'temperature': float(sample_temperature)}
        if cut_is_set(sample_top_k, sample_top_p):       # (only where set: a run without a cut writes the checkpoints it always wrote)
            sampling.update(top_k=int(sample_top_k), top_p=float(sample_top_p))
    elif cut_is_set(sample_top_k, sample_top_p):
        raise ValueError('sample_top_k / sample_top_p without sample_schedule: there is no pick to truncate')
    cut_keywords = {'top_k': sampling['top_k'], 'top_p': sampling['top_p']} if sampling is not None and 'top_k' in sampling else {}
    num_lines = s2s.map_files(filenames)
    s2s.logger.info('Training on "%d" files with %d lines', len(filenames), num_lines)
    if val_filenames:
        num_lines = s2s.map_files(val_filenames)
        s2s.logger.info('Validating on "%d" files with %d lines', len(val_filenames), num_lines)
        split_rand = None
    if teacher is not None:
        check_teacher(s2s, teacher, distill_k, distill_alpha)    # (after map_files: the student's mapping is final only now)
    if risk is not None and proposal is not None:
        check_risk(s2s, risk_samples, risk_alpha, risk_temperature, risk_top_k, risk_top_p, proposal, teacher, sample_schedule)
    state = resume_state(s2s, resume) if resume else None        # (after map_files: the mapping is part of what must match)
    if state is not None:
        check_distill_resume(state, resume, teacher, distill_k, distill_alpha)
        check_sampling_resume(state, resume, sampling)
        check_risk_resume(state, resume, risk)
    if val_filenames:
        if state is not None and state['split_rand'] is not None:
            raise ValueError('cannot resume from "%s": it was trained without validation files' % resume)
    else:
        s2s.logger.info('Validating on random 20% lines from those files')
        split_rand = s2s._rng.uniform(0, 1, (num_lines,)) if state is None else state['split_rand']
        if split_rand is None or len(split_rand) != num_lines:
            raise ValueError('cannot resume from "%s": it was trained with %s' % (
                resume, 'validation files' if split_rand is None else 'a split of %d lines, these files have %d' % (len(split_rand), num_lines)))
    if state is not None:
        _, layers = s2s._read_container(resume)          # the checkpoint's weights ...
        s2s._assign_layers(layers, keras_h5.layer_tensors(s2s.depth, s2s.bridge_dense, s2s.deep_bidirectional_encoder), skip_mismatch=False)
        s2s._rng.bit_generator.state = state['rng']      # ... and the generator as the next epoch found it
    rng = s2s._rng
    if sampling is not None:                 # the coins' seed: drawn once per run, a resumed run keeps its own
        sampling['seed'] = int(state['sample']['seed']) if state is not None else int(rng.integers(0, 2 ** 63))
    if risk is not None:                     # the candidates' seed, likewise
        risk['seed'] = int(state['risk']['seed']) if state is not None else int(rng.integers(0, 2 ** 63))
    engine = s2s._require_engine()
    engine.set_option('deterministic', 1 if s2s.deterministic else 0)
    teacher_engine = None
    if teacher is not None:
        teacher_engine = teacher._require_engine()
        teacher_engine.set_option('deterministic', 1 if s2s.deterministic else 0)      # (governs the scoring pass as it governs a step)
    own_proposal = None
    if risk is not None and proposal is None:        # a private copy of the model: its weights follow the training weights per epoch
        proposal = own_proposal = proposal_copy(s2s)
    adam = tuple(state['adam']) if state is not None else ADAM
    engine.train_begin(*adam, frozen=tuple(s2s.frozen_prefixes))
    if state is not None:
        engine.set_train_state(state['m'], state['v'], state['step'])
    step_id = int(state['step']) if state is not None else 0     # the session's step count: every mode-1 step adds one
    stop = {'flag': False}
    old_handler = None
    try:
        old_handler = signal.signal(signal.SIGINT, lambda *a: stop.__setitem__('flag', True))   # StopSignalCallback
    except ValueError:
        pass                                           # not in the main thread
    history = []
    best, best_weights, wait, best_epoch, first = np.inf, None, 0, 0, 0
    if state is not None:
        history = list(state['history'])
        best, wait, best_epoch, first = state['best_val_loss'], state['wait'], state['best_epoch'], state['epoch']
        if best_epoch:
            if set(state['best']) != set(engine.pshapes):
                raise ValueError('cannot resume from "%s": the best epoch\'s weights are missing' % resume)
            best_weights = {k: np.array(v) for k, v in state['best'].items()}
        if wait >= 3:                                  # the run ended there (EarlyStopping): nothing left to train
            s2s.logger.info('Epoch %05d: early stopping (at the checkpoint resumed from)', first)
            first = s2s.epochs
    try:
        for epoch in range(first, s2s.epochs):
            total, nb = 0.0, 0
            nan = cut = False
            ratio = schedule_ratio(sample_schedule, epoch, s2s.epochs) if sampling is not None else None
            if risk is not None:
                # every random draw of a minimum-risk epoch happens in this thread (risk_step): the worker only loads lines; the
                # lines' running numbers start at epoch * 2^32, so that a resumed run draws what the uninterrupted one drew
                if own_proposal is not None:
                    own_proposal.set_weights(engine.train_weights())
                settings = dict(risk, model=s2s, batch_size=s2s.batch_size, stream=epoch << 32, edit_costs=risk_costs)
                for batch in prefetch(line_batches(s2s, filenames, split_rand)):
                    losses = risk_step(engine, proposal, batch, settings, rng)
                    if not all(np.isfinite(losses)):
                        s2s.logger.warning('Batch %d: Invalid loss, terminating training', nb)
                        nan = True
                        break
                    total += sum(losses) / max(len(losses), 1); nb += 1
                    if stop['flag']:
                        cut = True
                        break
            # the next batches are vectorised by a worker thread while the device runs this one (kt:133-145)
            hard_batches = prefetch(train_batches(s2s, filenames, split_rand, rng)) if risk is None else ()
            for idx, val, dec_in, dec_out, w, masks in hard_batches:
                if teacher_engine is not None:
                    loss, _ = distill_step(engine, teacher_engine, (idx, val, dec_in, dec_out, w, masks), distill_k, distill_alpha)
                elif sampling is not None:
                    loss, _, _ = engine.train_step_sampled(idx, val, dec_in, dec_out, w, masks, mode=1, ratio=ratio, seed=sampling['seed'],
                                                           step_id=step_id, pick=sample_pick, passes=sample_passes,
                                                           temperature=sample_temperature, **cut_keywords)
                    step_id += 1
                else:
                    loss, _ = engine.train_step(idx, val, dec_in, dec_out, w, masks, mode=1)
                if not np.isfinite(loss):
                    s2s.logger.warning('Batch %d: Invalid loss, terminating training', nb)   # TerminateOnNaN
                    nan = True
                    break
                total += loss; nb += 1
                if stop['flag']:
                    cut = True                         # (the epoch is incomplete: see the checkpoint below)
                    break
            vtotal, vn = 0.0, 0
            if not nan:
                for idx, val, dec_in, dec_out, w in prefetch(validation_batches(s2s, val_filenames or filenames, split_rand)):
                    loss, _ = engine.train_step(idx, val, dec_in, dec_out, w, None, mode=0)
                    vtotal += loss; vn += 1
            val_loss = vtotal / vn if vn else float('nan')
            history.append({'loss': total / max(nb, 1), 'val_loss': val_loss})
            s2s.logger.info('epoch %d: loss %.4f val_loss %.4f (%d/%d batches)%s', epoch + 1, history[-1]['loss'], val_loss, nb, vn,
                            '' if ratio is None else ' sample ratio %.4f' % ratio)
            if nan or not np.isfinite(val_loss):
                break
            weights = engine.train_weights()
            if val_loss < best:
                best, best_weights, wait, best_epoch = val_loss, weights, 0, epoch + 1
            else:
                wait += 1
            # ModelCheckpoint("model.ckpt.weights-{epoch:02d}-{val_loss:.2f}.h5", save_weights_only=True), seq2seq.py:621-622 -- with
            # checkpoint_training_state, plus everything the next epoch starts from (keras_h5: the training-state group) -- only
            # after a whole epoch: a run stopped inside one resumes from the checkpoint before and trains the epoch again
            ckpt_state = None
            if s2s.checkpoint_training_state and not cut:
                m, v, step = engine.train_state()
                ckpt_state = {'epoch': epoch + 1, 'step': step, 'wait': wait, 'best_epoch': best_epoch, 'best_val_loss': best,
                              'adam': adam, 'frozen': list(s2s.frozen_prefixes), 'rng': rng.bit_generator.state,
                              'split_rand': split_rand, 'history': history, 'm': m, 'v': v, 'best': best_weights or {}}
                if teacher is not None:
                    ckpt_state['distill'] = (int(distill_k), float(distill_alpha))
                if sampling is not None:
                    ckpt_state['sample'] = dict(sampling)
                if risk is not None:
                    ckpt_state['risk'] = dict(risk)
            keras_h5.write_model('model.ckpt.weights-%02d-%.2f.h5' % (epoch + 1, val_loss), s2s._config_dict(), weights, ckpt_state)
            if wait >= 3:                              # EarlyStopping(patience=3, restore_best_weights)
                s2s.logger.info('Epoch %05d: early stopping', epoch + 1)
                break
            if stop['flag']:
                break
    finally:
        if old_handler is not None:
            signal.signal(signal.SIGINT, old_handler)
        engine.train_end()
        if teacher_engine is not None:
            teacher_engine.score_release()             # (the teacher's forward-only scoring state)
        if own_proposal is not None and own_proposal.engine is not None:
            own_proposal.engine.close()
            own_proposal.engine = None
    s2s.history = history
    if best_weights is not None:
        s2s.logger.info('training finished with val_loss %f', best)
        s2s._weights = {k: np.array(v) for k, v in best_weights.items()}
        s2s._dirty = True
        s2s.status = 2
    else:
        s2s.logger.critical('training failed')
        s2s._weights = engine.get_weights()
        s2s._dirty = True
        s2s.status = 1
