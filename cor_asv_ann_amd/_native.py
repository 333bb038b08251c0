"""ctypes binding of include/cor_asv_ann_hip.h (the C ABI of the HIP hot path).

There is no fallback: if the shared library is missing or a call fails, this raises.
"""
import ctypes
import os
from ctypes import (POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_uint64, c_void_p)

import numpy as np

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'lib', 'libcor_asv_ann_hip.so')
if os.environ.get('CASV_LIB_PATH'):          # measurement aid: A/B of two builds of the library on one box
    LIB_PATH = os.environ['CASV_LIB_PATH']

CASV_ERR_NAN = -5


class NativeError(RuntimeError):
    def __init__(self, code, message):
        super().__init__('cor_asv_ann_hip error %d: %s' % (code, message))
        self.code = code


class Config(Structure):
    _fields_ = [('depth', c_int32), ('width', c_int32), ('voc_size', c_int32), ('window_width', c_int32),
                ('residual_connections', c_int32), ('deep_bidirectional_encoder', c_int32),
                ('bridge_dense', c_int32), ('lm', c_int32), ('stateful', c_int32)]


class AdamParams(Structure):
    _fields_ = [('lr', c_float), ('beta1', c_float), ('beta2', c_float), ('epsilon', c_float), ('clipnorm', c_float)]


class BeamParams(Structure):
    _fields_ = [('batch_size', c_int32), ('beam_width_in', c_int32), ('beam_width_out', c_int32),
                ('max_results', c_int32), ('beam_threshold_in', c_double), ('rejection_threshold', c_double),
                ('cost0', c_double)]


class SampleParams(Structure):
    _fields_ = [('seed', c_uint64), ('temperature', c_float), ('top_k', c_int32), ('samples', c_int32)]


class SampleCut(Structure):
    """casv_sample_cut: the truncation of a sampled pick, top_k in 0 .. 4095 (0 = none) and top_p in (0, 1] (1 = none)"""
    _fields_ = [('top_k', c_int32), ('top_p', c_float)]


class EditCosts(Structure):
    """casv_edit_costs: what an insertion or deletion, a substitution and a substitution within one key cost, and the cost of one
    full edit that mode 1 divides by"""
    _fields_ = [('gap', c_int32), ('sub', c_int32), ('near', c_int32), ('unit', c_int32)]


class SchedParams(Structure):
    _fields_ = [('seed', c_uint64), ('step_id', c_uint64), ('ratio', c_float), ('temperature', c_float), ('pick', c_int32),
                ('passes', c_int32)]


class DebugRows(Structure):
    """casv_debug_rows: an input of casv_debug_gemm_jobs whose rows move with the step (K segment, cell state, zinit)"""
    _fields_ = [('pool', c_void_p), ('rows', c_void_p), ('first', c_void_p), ('slots', c_int32), ('pool_rows', c_int32),
                ('ld', c_int32), ('width', c_int32), ('koff', c_int32), ('step_mul', c_int32), ('step_add', c_int32),
                ('skip_first', c_int32)]


class DebugOut(Structure):
    _fields_ = [('data', c_void_p), ('slots', c_int32), ('ld', c_int32), ('step_mul', c_int32), ('step_add', c_int32)]


class DebugJob(Structure):
    _fields_ = [('M', c_int32), ('N', c_int32), ('Ktot', c_int32), ('nseg', c_int32), ('a', DebugRows * 3), ('c_in', DebugRows),
                ('zinit', DebugRows), ('Bt', c_void_p), ('bias', c_void_p), ('out', DebugOut), ('c_out', DebugOut),
                ('gates_out', DebugOut), ('out2', DebugOut), ('nact', c_void_p), ('nact_lines', c_int32), ('nact_group', c_int32),
                ('b_static', c_int32), ('epi_plain', c_int32)]


class DebugSum(Structure):
    """casv_debug_sum: the train step's launch fields of one job (casv_debug_gemm_jobs_sum)"""
    _fields_ = [('ksplit', c_int32), ('kgroups', c_int32), ('accumulate', c_int32), ('out_zeroed', c_int32)]


class DebugBwdJob(Structure):
    """casv_debug_bwd_job: one layer's backward time step (casv_debug_bwd_step)"""
    _fields_ = [('rows', c_int32), ('W', c_int32), ('N', c_int32), ('Bt', c_void_p), ('a', c_void_p), ('lda', c_int64), ('mask_a', c_void_p),
                ('b', c_void_p), ('ldb', c_int64), ('c', c_void_p), ('ldc', c_int64), ('c_prev', c_void_p), ('ld_cprev', c_int64),
                ('gates', c_void_p), ('cell', c_void_p), ('dc_in', c_void_p), ('dz', c_void_p), ('dc', c_void_p), ('out', c_void_p),
                ('ld_out', c_int64)]


# what every casv_train_step* entry begins with: handle, mode, B, T, U, A, then enc_idx, enc_val, dec_in
_STEP = [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]
# ... the hard-target entries go on with dec_out, weights and the three masks
_STEP_HARD = _STEP + [c_void_p] * 5

# name -> (restype, argtypes); every symbol declared in the header is listed here and checked at load
SIGNATURES = {
    'casv_last_error': (c_char_p, []),
    'casv_device_count': (c_int, []),
    'casv_version': (c_char_p, []),
    'casv_model_create': (c_int, [POINTER(Config), c_int, POINTER(c_void_p)]),
    'casv_model_destroy': (None, [c_void_p]),
    'casv_set_weight': (c_int, [c_void_p, c_char_p, c_void_p, c_int64]),
    'casv_get_weight': (c_int, [c_void_p, c_char_p, c_void_p, c_int64]),
    'casv_commit_weights': (c_int, [c_void_p]),
    'casv_encode': (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    'casv_set_encoder_outputs': (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    'casv_get_encoder_outputs': (c_int, [c_void_p, c_void_p, c_void_p]),
    'casv_decoder_step': (c_int, [c_void_p, c_int32] + [c_void_p] * 7),
    'casv_decoder_step_lm': (c_int, [c_void_p, c_int32] + [c_void_p] * 8),
    'casv_decode_greedy': (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    'casv_decode_beam': (c_int, [c_void_p, POINTER(BeamParams), c_int32] + [c_void_p] * 8),
    'casv_decode_sample': (c_int, [c_void_p, POINTER(SampleParams), c_int32] + [c_void_p] * 6),
    'casv_debug_sample_rows': (c_int, [c_void_p, c_int32, c_int32, POINTER(SampleParams), c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_float] + [c_void_p] * 4),
    'casv_decode_sample_cut': (c_int, [c_void_p, POINTER(SampleParams), POINTER(SampleCut), c_int32] + [c_void_p] * 6),
    'casv_debug_sample_cut_rows': (c_int, [c_void_p, c_int32, c_int32, POINTER(SampleParams), POINTER(SampleCut), c_int32, c_void_p, c_void_p,
                                           c_void_p, c_void_p, c_float] + [c_void_p] * 4),
    'casv_train_begin': (c_int, [c_void_p, POINTER(AdamParams), c_char_p]),
    'casv_train_step': (c_int, _STEP_HARD + [POINTER(c_double)] * 2),
    'casv_train_get_gradient': (c_int, [c_void_p, c_char_p, c_void_p, c_int64]),
    'casv_train_get_state': (c_int, [c_void_p, c_char_p, c_int32, c_void_p, c_int64]),
    'casv_train_set_state': (c_int, [c_void_p, c_char_p, c_int32, c_void_p, c_int64]),
    'casv_train_get_step': (c_int, [c_void_p, POINTER(c_int64)]),
    'casv_train_set_step': (c_int, [c_void_p, c_int64]),
    'casv_train_sync_weights': (c_int, [c_void_p]),
    'casv_train_end': (c_int, [c_void_p]),
    'casv_score_targets': (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32] + [c_void_p] * 10),
    'casv_score_candidates': (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32] + [c_void_p] * 10),
    'casv_score_get_alignments_sparse': (c_int, [c_void_p, c_int32, c_void_p, c_void_p]),
    'casv_score_get_alternatives': (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    'casv_score_release': (c_int, [c_void_p]),
    'casv_consensus': (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32] + [c_void_p] * 6),
    'casv_consensus_align': (c_int, [c_void_p, c_int32, c_int32, c_int32] + [c_void_p] * 5),
    'casv_consensus_costed': (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32] + [c_void_p] * 4 + [POINTER(EditCosts)] + [c_void_p] * 3),
    'casv_consensus_align_costed': (c_int, [c_void_p, c_int32, c_int32, c_int32] + [c_void_p] * 4 + [POINTER(EditCosts)] + [c_void_p] * 2),
    'casv_consensus_vote': (c_int, [c_void_p, c_int32] + [c_void_p] * 4),
    'casv_debug_set_align_budget': (c_int, [c_void_p, c_int64]),
    'casv_train_step_soft': (c_int, _STEP + [c_int32] + [c_void_p] * 6 + [POINTER(c_double)] * 2),
    'casv_train_step_sampled': (c_int, _STEP_HARD + [POINTER(SchedParams), c_void_p] + [POINTER(c_double)] * 2),
    'casv_debug_sched_rows': (c_int, [c_void_p, c_int32, c_int32, POINTER(SchedParams)] + [c_void_p] * 4 + [c_float, c_void_p]),
    'casv_train_step_sampled_cut': (c_int, _STEP_HARD + [POINTER(SchedParams), POINTER(SampleCut), c_void_p] + [POINTER(c_double)] * 2),
    'casv_debug_sched_cut_rows': (c_int, [c_void_p, c_int32, c_int32, POINTER(SchedParams), POINTER(SampleCut)] + [c_void_p] * 4
                                  + [c_float, c_void_p]),
    'casv_debug_soft_ce_rows': (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float,
                                        c_int32, POINTER(c_double), c_void_p, c_int32]),
    'casv_train_step_risk': (c_int, _STEP_HARD + [c_int32, c_void_p, c_double, c_void_p, c_void_p] + [POINTER(c_double)] * 2),
    'casv_debug_risk_rows': (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_double,
                                     c_float, c_int32, POINTER(c_double), c_void_p, c_void_p, c_void_p]),
    'casv_debug_score_rows': (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    'casv_debug_alternatives_rows': (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    'casv_profile': (c_int, [c_void_p, c_int32]),
    'casv_profile_read': (c_int, [c_void_p, c_char_p, POINTER(c_int64), POINTER(c_double), POINTER(c_double),
                                  POINTER(c_double)]),
    'casv_debug_gemm': (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, POINTER(c_double)]),
    'casv_debug_contract': (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    'casv_debug_contract_tn': (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_int64,
                                       c_void_p, c_int64, c_void_p]),
    'casv_debug_activation': (c_int, [c_void_p, c_int32, c_int64, c_void_p, c_void_p]),
    'casv_debug_gemm_jobs': (c_int, [c_void_p, c_int32, c_int32, POINTER(DebugJob), c_int32, c_int32]),
    'casv_debug_gemm_jobs_acc': (c_int, [c_void_p, c_int32, c_int32, POINTER(DebugJob), POINTER(DebugRows), c_int32, c_int32]),
    'casv_debug_gemm_jobs_sum': (c_int, [c_void_p, c_int32, c_int32, POINTER(DebugJob), POINTER(DebugSum), c_int32, c_int32, c_int32]),
    'casv_debug_get_u': (c_int, [c_void_p, c_void_p]),
    'casv_debug_bwd_step': (c_int, [c_void_p, c_int32, c_int32, POINTER(DebugBwdJob)]),
    'casv_set_option': (c_int, [c_void_p, c_char_p, c_int64]),
    'casv_get_alignments_sparse': (c_int, [c_void_p, c_int32, c_void_p, c_void_p]),
    'casv_comm_unique_id': (c_int, [c_void_p]),
    'casv_comm_init': (c_int, [c_void_p, c_int32, c_int32, c_void_p]),
    'casv_comm_all_gather': (c_int, [c_void_p, c_void_p, c_void_p, c_int64]),
    'casv_comm_all_reduce_max': (c_int, [c_void_p, POINTER(c_double)]),
    'casv_comm_destroy': (c_int, [c_void_p]),
    'casv_records_reset': (c_int, [c_void_p, c_int32, c_int32]),
    'casv_records_append': (c_int, [c_void_p, c_int32]),
    'casv_records_read': (c_int, [c_void_p, c_void_p]),
    'casv_records_device_ptr': (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_int64)]),
    'casv_comm_all_gather_records': (c_int, [c_void_p, c_void_p]),
    'casv_get_stat': (c_int, [c_void_p, c_char_p, POINTER(c_int64)]),
    'casv_realign_path': (c_int, [c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_float, c_void_p, POINTER(c_double)]),
    'casv_synchronize': (c_int, [c_void_p]),
}

_lib = None


def load():
    """Load the HIP library (once).  Raises if it has not been built (`python -c 'import
    __graft_entry__ as g; g.build()'` or `make -C cor_asv_ann_amd/csrc`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError('HIP library %s not found: build it with `make -C cor_asv_ann_amd/csrc` '
                           '(there is no CPU fallback)' % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        if (os.environ.get('CASV_LIB_PATH') and (name.startswith('casv_debug_') or name.endswith('_cut') or name.startswith('casv_consensus'))
                and not hasattr(lib, name)):
            continue                     # (A/B against an older build of the library: it may lack a test-support entry, the cut entries, the vote or the confusion network)
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def check(code):
    if code != 0:
        raise NativeError(code, load().casv_last_error().decode('utf-8', 'replace'))


def ptr(a):
    return None if a is None else a.ctypes.data_as(c_void_p)


def carray(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)
