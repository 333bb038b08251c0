"""Source checks of the decode host code (csrc/decode.hip): what the split into a step view, named launches and phases promises
stays true of the text -- no call state in the handle, no recursion, one place that fills the attention's shared arguments."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'cor_asv_ann_amd', 'csrc')


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _definitions(text):
    """{first line of a top-level definition: its lines}: from a line at column 0 that is no comment, directive or closing brace
    to the next closing brace at column 0."""
    out, head, body = {}, None, []
    for line in text.split('\n'):
        if head is None:
            if line and not line[0].isspace() and not line.startswith(('//', '#', '}')):
                head, body = line, []
        if head is not None:
            body.append(line)
            if line.startswith('}') or (line is head and line.rstrip().endswith((';', '}'))):          # (or a one-liner)
                out[head] = body
                head = None
    return out


def test_the_skip_is_call_state_and_the_redo_a_loop():
    assert 'skip_nact' not in _src('engine.h') and 'skip_group' not in _src('engine.h')
    decode = _src('decode.hip')
    assert decode.count('casv_decode_beam(') == 1                       # the definition: no call inside the file
    assert 'skip_nact' not in decode and '__global__' not in decode
    assert '#define ENS' not in decode and '#define ENS' not in _src('engine.hip')


def test_one_function_fills_the_shared_attention_arguments():
    holders = [head for head, body in _definitions(_src('decode.hip')).items() if 'AttnArgs a{}' in '\n'.join(body)]
    assert len(holders) == 1 and holders[0].startswith('static AttnArgs attention_args(const casv_model* m)')
    for other in ('engine.hip',):
        assert 'AttnArgs' not in _src(other)


def test_the_step_is_a_short_list_of_launches_from_one_view():
    defs = _definitions(_src('decode.hip'))
    assert 'static void launch_step(casv_model* m, const DecodeStep& st) {' in defs
    longest = max(defs.values(), key=len)
    assert len(longest) <= 90, (longest[0], len(longest))
    # the order of a step's launches
    step = '\n'.join(defs['static void launch_step(casv_model* m, const DecodeStep& st) {'])
    marks = ['layer_gemm(m, st, 1)', 'step_attention(m, st)', 'layer_gemm(m, st, n)', 'top_gemm(m, st)', 'projection_gemm(m, st)',
             'step_softmax(m, st)']
    at = [step.index(x) for x in marks]
    assert at == sorted(at)
    # the step number and the live rows are stamped on a GEMM's arguments in one place
    assert len(re.findall(r'\.nact_group = ', _src('decode.hip'))) == 3        # stamp, attention, softmax


def test_what_moved_and_what_stayed():
    engine, decode = _src('engine.hip'), _src('decode.hip')
    for name in ('decode_buffers_signature', 'ensure_session', 'init_root', 'launch_step', 'decoder_step', 'persist_applies',
                 'decode_greedy_persistent'):
        assert re.search(r'^(static )?[\w ]+ %s\(' % name, decode, re.M), name
        assert not re.search(r'^(static )?[\w ]+ %s\(' % name, engine, re.M), name
    assert 'struct StepRunner {' in decode and 'StepRunner' not in engine
    for entry in ('casv_decode_greedy', 'casv_decode_beam', 'casv_get_alignments_sparse', 'casv_decoder_step', 'casv_decoder_step_lm'):
        assert 'extern "C" int %s(' % entry in decode and entry + '(' not in engine
    for entry in ('casv_model_create', 'casv_model_destroy', 'casv_commit_weights', 'casv_records_append', 'casv_get_stat',
                  'casv_profile', 'casv_debug_gemm', 'casv_debug_gemm_jobs', 'casv_set_option', 'casv_synchronize'):
        assert 'extern "C" int %s(' % entry in engine or 'extern "C" void %s(' % entry in engine
    assert 'm->Vp = (cfg->voc_size + 31) & ~31;' in engine
    with open(os.path.join(CSRC, 'Makefile')) as f:
        assert ' decode.hip ' in re.search(r'^SRCS = (.*)$', f.read(), re.M).group(0)
