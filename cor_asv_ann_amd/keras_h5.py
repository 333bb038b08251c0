"""The reference's model container: Keras-2.3 `save_weights` HDF5 layout + the `config` group.

Layout (keras/engine/saving.py `save_weights_to_hdf5_group`, Keras 2.3.1, restated; the reference calls it
at seq2seq.py:1129 and adds the `config` group at seq2seq.py:1130-1141):

    /                         attrs: layer_names (fixed-length byte strings), backend, keras_version
    /<layer>/                 attrs: weight_names, in `layer.weights` order
    /<layer>/<weight name>    one float32 dataset per weight; the weight name contains '/', so it lives in a
                              nested group, e.g. /encoder_lstm_1/encoder_lstm_1/forward_encoder_lstm_1/kernel:0
    /config/{width,depth,stateful,residual_connections,deep_bidirectional_encoder,bridge_dense}  scalars
    /config/mapping           uint32[voc_size]: code point of every index, 0 = unmapped

Loading is by layer name and, inside a layer, by ORDER of `weight_names` (keras `load_weights(by_name=True)`,
seq2seq.py:1172): the names themselves only address the datasets.  Layers trained with CuDNNLSTM on a GPU
carry the cuDNN weight format (bias of 8W); `_from_cudnn` restates keras' `_convert_rnn_weights`.

Tensor names on this side are those of `engine.weight_shapes`.

Optional training state (this package only; `write_model(..., state=...)`, read by `read_training_state`): a group beside the
layers that is not named in `layer_names`, so that keras' `load_weights` and this package's loaders never look at it:

    /training_state/format                      int64 scalar (1)
    /training_state/{epoch,step,wait,best_epoch}  int64 scalars: completed epochs, Adam's step count, EarlyStopping patience
                                                counter and the epoch of the best val_loss (0: none yet)
    /training_state/best_val_loss               float64 scalar (inf: none yet)
    /training_state/adam                        float64[5]: lr, beta1, beta2, epsilon, clipnorm
    /training_state/frozen                      bytes: the frozen tensor-name prefixes, comma-separated
    /training_state/{distill_k,distill_alpha}   int64 / float64 scalars: a distilled run's K and alpha (absent: no teacher)
    /training_state/sample                      bytes: JSON of a scheduled-sampling run's settings {seed, schedule, pick, passes,
                                                temperature} (absent: no sample_schedule)
    /training_state/risk                        bytes: JSON of a minimum-risk run's settings {seed, samples, alpha, temperature, top_k,
                                                top_p, own_proposal} (absent: no risk_samples)
    /training_state/rng                         bytes: JSON of the numpy bit generator's state
    /training_state/split_rand                  float64[lines]: the validation split (absent: validation files were given)
    /training_state/history_{loss,val_loss}     float64[epochs]
    /training_state/m/<tensor>, .../v/<tensor>  float32: Adam's moments of every trained tensor (names as in the layers)
    /training_state/best/<tensor>               float32: the best epoch's weights (EarlyStopping(restore_best_weights))
"""
import json
from collections import OrderedDict

import numpy as np

from . import hdf5


def _bridge(out, n, names):
    """The bridge_dense layers of encoder layer n (seq2seq.py:299-301): Dense(width, tanh) 'bridge_h_<n>', 'bridge_c_<n>'."""
    for part in ('h', 'c'):
        out['bridge_%s_%d' % (part, n)] = (['bridge_%s_%d/kernel:0' % (part, n), 'bridge_%s_%d/bias:0' % (part, n)] if names
                                            else ['bridge%d_%s_K' % (n, part), 'bridge%d_%s_b' % (n, part)])


def layer_tensors(depth, bridge_dense=False, deep=False):
    """Ordered {keras layer name: [tensor names in layer.weights order]} (seq2seq.py:239-350, attention.py:418-421,598-609)."""
    d = int(depth)
    out = OrderedDict()
    out['char_input_projection'] = ['E']
    out['encoder_lstm_1'] = ['enc1_%s_%s' % (direction, part) for direction in ('fw', 'bw') for part in 'KRb']
    if bridge_dense:
        _bridge(out, 1, False)
    for n in range(2, d + 1):
        out['encoder_lstm_%d' % n] = (['enc%d_%s_%s' % (n, direction, part) for direction in ('fw', 'bw') for part in 'KRb'] if deep
                                      else ['enc%d_%s' % (n, part) for part in 'KRb'])
        if bridge_dense:
            _bridge(out, n, False)
    out['attention_dense'] = ['att_U']
    for n in range(1, d):
        out['decoder_lstm_%d' % n] = ['dec%d_%s' % (n, part) for part in 'KRb']
    out['decoder_lstm_%d' % d] = ['att_Wa', 'att_va', 'att_bUW', 'att_bv'] + ['dec%d_%s' % (d, part) for part in 'KRb']
    return out


def _keras_weight_names(depth, bridge_dense=False, deep=False):
    """Variable names keras/TF1 gives the weights (`<scope>/<name>:0`), per layer, in order."""
    d = int(depth)
    lstm = ['kernel:0', 'recurrent_kernel:0', 'bias:0']
    out = OrderedDict()
    out['char_input_projection'] = ['char_input_projection/kernel:0']
    out['encoder_lstm_1'] = ['encoder_lstm_1/%s_encoder_lstm_1/%s' % (direction, w)
                             for direction in ('forward', 'backward') for w in lstm]
    if bridge_dense:
        _bridge(out, 1, True)
    for n in range(2, d + 1):
        out['encoder_lstm_%d' % n] = (['encoder_lstm_%d/%s_encoder_lstm_%d/%s' % (n, direction, n, w) for direction in ('forward', 'backward') for w in lstm]
                                      if deep else ['encoder_lstm_%d/%s' % (n, w) for w in lstm])
        if bridge_dense:
            _bridge(out, n, True)
    out['attention_dense'] = ['attention_dense/kernel:0']
    for n in range(1, d):
        out['decoder_lstm_%d' % n] = ['decoder_lstm_%d/%s' % (n, w) for w in lstm]
    out['decoder_lstm_%d' % d] = ['decoder_lstm_%d/%s' % (d, w) for w in ['W_a:0', 'v_a:0', 'b_UW:0', 'b_v:0'] + lstm]
    return out


def _from_cudnn(kernel, recurrent, bias):
    """CuDNNLSTM -> LSTM weights (keras/engine/saving.py `_convert_rnn_weights`, n_gates = 4): every gate block of
    the kernels is stored transposed in Fortran order, and the input and recurrent biases are separate."""
    def per_gate(mat, func):
        return np.hstack([func(k) for k in np.hsplit(mat, 4)])
    kernel = per_gate(kernel, lambda k: k.T.reshape(k.shape, order='F'))
    recurrent = per_gate(recurrent, lambda k: k.T)
    bias = np.sum(np.split(bias, 2, axis=0), axis=0)
    return kernel, recurrent, bias


def _as_names(attr):
    if attr is None:
        return None
    return [n.decode('utf-8') if isinstance(n, bytes) else str(n) for n in np.asarray(attr).ravel().tolist()]


def _guard(func):
    """Truncated or damaged files surface as hdf5.H5Error, not as struct/index errors from the parser."""
    import functools
    import struct
    from zlib import error as zlib_error

    @functools.wraps(func)
    def wrapper(*args, **kwargs):
        try:
            return func(*args, **kwargs)
        except (struct.error, IndexError, ValueError, OverflowError, UnicodeDecodeError, RecursionError, MemoryError, zlib_error) as err:
            raise hdf5.H5Error('damaged or unsupported HDF5 file "%s": %s' % (args[0] if args else '?', err))
    return wrapper


@_guard
def read_config(filename):
    """The `config` group as a dict (seq2seq.py:1143-1162); {} if the file has none (plain keras weight files)."""
    with hdf5.File(filename) as f:
        root = f
        if 'config' not in root and 'model_weights' in root and 'config' in root['model_weights']:
            root = root['model_weights']
        if 'config' not in root:
            return {}
        cfg = root['config']
        out = {}
        for key in cfg.keys():
            node = cfg[key]
            if isinstance(node, hdf5.Dataset):
                out[key] = node.read()
        return out


@_guard
def read_layers(filename):
    """{keras layer name: [arrays in weight_names order]} for every layer group that has weights."""
    with hdf5.File(filename) as f:
        root = f
        if 'layer_names' not in root.attrs and 'model_weights' in root:        # full `model.save` files (seq2seq.py:1186-1187)
            root = root['model_weights']
        names = _as_names(root.attrs.get('layer_names'))
        if names is None:
            names = [k for k in root.keys() if k != 'config']
        layers = OrderedDict()
        for lname in names:
            if lname not in root:
                continue
            g = root[lname]
            if not isinstance(g, hdf5.Group):
                continue
            wnames = _as_names(g.attrs.get('weight_names'))
            if wnames is None:
                wnames = [p for p, _ in g.visit_datasets()]
            arrays = [np.asarray(g[w].read(), np.float32) for w in wnames]
            if arrays:
                layers[lname] = arrays
        return layers


def layers_to_tensors(layers, logger=None):
    """Keras layer weight lists -> {tensor name: array}, keyed per layer: {layer: {tensor: array}}.
    The attention cell is recognised by its 7 weights, Bidirectional by 6, plain LSTM by 3."""
    out = OrderedDict()
    for lname, arrays in layers.items():
        arrays = list(arrays)
        if lname in ('char_input_projection', 'attention_dense') and len(arrays) == 1:
            out[lname] = OrderedDict([('E' if lname == 'char_input_projection' else 'att_U', arrays[0])])
            continue
        if (lname.startswith('bridge_h_') or lname.startswith('bridge_c_')) and len(arrays) == 2:
            try:
                n = int(lname.rsplit('_', 1)[1])
            except ValueError:
                continue
            part = lname[len('bridge_')]
            out[lname] = OrderedDict([('bridge%d_%s_K' % (n, part), arrays[0]), ('bridge%d_%s_b' % (n, part), arrays[1].reshape(-1))])
            continue
        if not (lname.startswith('encoder_lstm_') or lname.startswith('decoder_lstm_')):
            continue
        try:
            n = int(lname.rsplit('_', 1)[1])
        except ValueError:
            continue
        prefix = ('enc%d' if lname.startswith('encoder') else 'dec%d') % n
        tensors = OrderedDict()
        if len(arrays) == 7:
            tensors['att_Wa'], tensors['att_va'], tensors['att_bUW'], tensors['att_bv'] = arrays[:4]
            tensors['att_va'] = tensors['att_va'].reshape(-1)
            arrays = arrays[4:]
        groups = [('', arrays)]
        if len(arrays) == 6:
            groups = [('_fw', arrays[:3]), ('_bw', arrays[3:])]
        elif len(arrays) != 3:
            if logger:
                logger.warning('layer "%s" has %d weights, expected 3, 6 or 7: skipped', lname, len(arrays))
            continue
        for suffix, (k, r, b) in groups:
            units = r.shape[0]
            if b.shape == (8 * units,):
                k, r, b = _from_cudnn(k, r, b)
            tensors[prefix + suffix + '_K'], tensors[prefix + suffix + '_R'], tensors[prefix + suffix + '_b'] = k, r, b
        out[lname] = tensors
    return out


def read_model(filename, logger=None):
    """(config dict, {layer: {tensor: array}})."""
    return read_config(filename), layers_to_tensors(read_layers(filename), logger)


def write_model(filename, config, weights, state=None):
    """Write `weights` ({tensor name: array}, all tensors of the model) and `config` in the reference's layout;
    `state` (a dict as read_training_state returns it, or None): the optional training-state group as well."""
    depth = int(config['depth'])
    bridge = bool(np.asarray(config.get('bridge_dense', False)).item()) if 'bridge_dense' in config else False
    deep = bool(np.asarray(config.get('deep_bidirectional_encoder', False)).item()) if 'deep_bidirectional_encoder' in config else False
    table, knames = layer_tensors(depth, bridge, deep), _keras_weight_names(depth, bridge, deep)
    w = hdf5.Writer()
    w.set_attr('/', 'layer_names', np.array([n.encode('utf-8') for n in table], dtype='S'))
    w.set_attr('/', 'backend', np.bytes_(b'tensorflow'))
    w.set_attr('/', 'keras_version', np.bytes_(b'2.3.1'))
    for lname, tensors in table.items():
        w.create_group(lname)
        w.set_attr(lname, 'weight_names', np.array([n.encode('utf-8') for n in knames[lname]], dtype='S'))
        for tname, kname in zip(tensors, knames[lname]):
            a = np.asarray(weights[tname], np.float32)
            if tname == 'att_va':
                a = a.reshape(-1, 1)                    # attention.py:600
            w.create_dataset(lname + '/' + kname, a)
    for key, value in config.items():
        w.create_dataset('config/' + key, np.asarray(value))
    if state is not None:
        _write_state(w, state)
    w.save(filename)


STATE = 'training_state'


def _write_state(w, st):
    g = STATE + '/'
    w.create_group(STATE)
    w.create_dataset(g + 'format', np.asarray(1, np.int64))
    for key in ('epoch', 'step', 'wait', 'best_epoch'):
        w.create_dataset(g + key, np.asarray(int(st[key]), np.int64))
    w.create_dataset(g + 'best_val_loss', np.asarray(float(st['best_val_loss']), np.float64))
    w.create_dataset(g + 'adam', np.asarray(st['adam'], np.float64).reshape(5))
    w.create_dataset(g + 'frozen', np.bytes_(','.join(st['frozen']).encode('utf-8') or b','))
    w.create_dataset(g + 'rng', np.bytes_(json.dumps(st['rng']).encode('utf-8')))
    if st.get('distill') is not None:
        w.create_dataset(g + 'distill_k', np.asarray(int(st['distill'][0]), np.int64))
        w.create_dataset(g + 'distill_alpha', np.asarray(float(st['distill'][1]), np.float64))
    if st.get('sample') is not None:
        w.create_dataset(g + 'sample', np.bytes_(json.dumps(st['sample'], sort_keys=True).encode('utf-8')))
    if st.get('risk') is not None:
        w.create_dataset(g + 'risk', np.bytes_(json.dumps(st['risk'], sort_keys=True).encode('utf-8')))
    if st.get('split_rand') is not None:
        w.create_dataset(g + 'split_rand', np.asarray(st['split_rand'], np.float64))
    hist = st.get('history') or []
    if hist:
        w.create_dataset(g + 'history_loss', np.asarray([h['loss'] for h in hist], np.float64))
        w.create_dataset(g + 'history_val_loss', np.asarray([h['val_loss'] for h in hist], np.float64))
    for sub in ('m', 'v', 'best'):
        tensors = st.get(sub) or {}
        w.create_group(g + sub)
        for name, a in tensors.items():
            w.create_dataset(g + sub + '/' + name, np.asarray(a, np.float32))


@_guard
def read_training_state(filename):
    """The training-state group of a checkpoint as a dict (the keys write_model's `state` takes), or None if it has none."""
    with hdf5.File(filename) as f:
        if STATE not in f:
            return None
        g = f[STATE]
        fmt = int(np.asarray(g['format'].read()))
        if fmt != 1:
            raise hdf5.H5Error('training state of "%s" has format %d, this package reads format 1' % (filename, fmt))
        text = lambda key: bytes(np.asarray(g[key].read()).reshape(-1)[0]).decode('utf-8')
        st = {key: int(np.asarray(g[key].read())) for key in ('epoch', 'step', 'wait', 'best_epoch')}
        st['best_val_loss'] = float(np.asarray(g['best_val_loss'].read()))
        st['adam'] = [float(x) for x in np.asarray(g['adam'].read(), np.float64).reshape(5)]
        st['frozen'] = [p for p in text('frozen').split(',') if p]
        st['rng'] = json.loads(text('rng'))
        st['split_rand'] = np.asarray(g['split_rand'].read(), np.float64) if 'split_rand' in g else None
        if 'distill_k' in g:           # (a distilled run only: a plain run's state has the keys it always had)
            st['distill'] = (int(np.asarray(g['distill_k'].read())), float(np.asarray(g['distill_alpha'].read())))
        if 'sample' in g:              # (a scheduled-sampling run only)
            st['sample'] = json.loads(text('sample'))
        if 'risk' in g:                # (a minimum-risk run only)
            st['risk'] = json.loads(text('risk'))
        st['history'] = []
        if 'history_loss' in g:
            st['history'] = [{'loss': float(a), 'val_loss': float(b)} for a, b in
                             zip(np.asarray(g['history_loss'].read()).reshape(-1), np.asarray(g['history_val_loss'].read()).reshape(-1))]
        for sub in ('m', 'v', 'best'):
            st[sub] = OrderedDict()
            if sub in g:
                for name in g[sub].keys():
                    st[sub][name] = np.asarray(g[sub][name].read(), np.float32)
        return st
