"""ctypes binding of libfsmg -- exactly the entry points declared in include/fsmg.h.

This is "the reference-side binding a maintainer would add" (INTEGRATION.md): the
`models.lstm_baseline.LSTMBaseline` plugin calls these instead of a TensorFlow session.
"""
import ctypes as C
import os

import numpy as np

from fsmg.build import LIB

FSMG_GRAD_TAIL = 16
CLIP_MODES = {'tf1_slices': 0, 'dense': 1}
FSMG_CONFIG_VERSION = 4
GEMM_KINDS = {'auto': 0, 'bx3': 1, 'f32': 2}
SCHEDULES = {'auto': 0, 'single_stream': 1, 'two_stream': 2, 'xcd_partitioned': 3}
RECURRENCES = {'auto': 0, 'per_step': 1, 'column_split': 2, 'xcd_local': 3}

ERRORS = {-1: 'FSMG_ERR_INVALID', -2: 'FSMG_ERR_NO_DEVICE', -3: 'FSMG_ERR_HIP', -4: 'FSMG_ERR_NOMEM',
          -5: 'FSMG_ERR_NAME', -6: 'FSMG_ERR_SIZE', -7: 'FSMG_ERR_TOKEN_RANGE', -8: 'FSMG_ERR_STATE',
          -9: 'FSMG_ERR_TIMEOUT', -10: 'FSMG_ERR_SOFTMAX_RANGE'}
# the step was skipped on the device and the handle has changed how it runs the next one: repeat the call (include/fsmg.h)
RETRY_CODES = (-9, -10)


class FsmgError(RuntimeError):
    def __init__(self, code, message):
        super(FsmgError, self).__init__('%s: %s' % (ERRORS.get(code, code), message))
        self.code = code


class FsmgConfig(C.Structure):
    _fields_ = [('input_size', C.c_int32), ('max_len', C.c_int32), ('embedding_size', C.c_int32),
                ('hidden_size', C.c_int32), ('n_layers', C.c_int32), ('lr', C.c_float),
                ('max_grad_norm', C.c_float), ('n_decay', C.c_float), ('clip_norm_mode', C.c_int32),
                ('device', C.c_int32), ('max_sequences', C.c_int32), ('use_graph', C.c_int32),
                ('stream', C.c_void_p), ('state_arena', C.c_void_p), ('state_arena_bytes', C.c_uint64),
                ('config_version', C.c_int32), ('gemm', C.c_int32), ('schedule', C.c_int32), ('recurrence', C.c_int32),
                ('dp_split_backward', C.c_int32), ('reserved', C.c_int32 * 7)]


class FsmgStats(C.Structure):
    _fields_ = [('timeouts', C.c_int64), ('steps_skipped_timeout', C.c_int64), ('steps_skipped_token_range', C.c_int64),
                ('xcd_launches', C.c_int64), ('persistent_launches', C.c_int64), ('step_launches', C.c_int64),
                ('persistent_path', C.c_int32), ('fallback_steps_left', C.c_int32), ('steps_skipped_peer_failure', C.c_int64),
                ('xov_selfcheck_mismatches', C.c_int64), ('softmax_range_rows', C.c_int64), ('steps_skipped_softmax_range', C.c_int64),
                ('aux_stream_tries', C.c_int32), ('reserved0', C.c_int32)]


FSMG_GEN_CONFIG_VERSION = 1


class FsmgGenConfig(C.Structure):
    _fields_ = [('version', C.c_int32), ('n_seq', C.c_int32), ('num', C.c_int32), ('primer_len', C.c_int32),
                ('temperature', C.c_float), ('top_k', C.c_int32), ('seed', C.c_uint64), ('primer_on_device', C.c_int32),
                ('reserved', C.c_int32 * 7)]


FSMG_GEN_FILTERS_VERSION = 1


class FsmgGenFilters(C.Structure):
    _fields_ = [('version', C.c_int32), ('top_p', C.c_float), ('min_p', C.c_float), ('repetition_penalty', C.c_float),
                ('repeat_window', C.c_int32), ('reserved', C.c_int32 * 8)]


FSMG_CONSTRAINT_CONFIG_VERSION = 1


class FsmgConstraintConfig(C.Structure):
    _fields_ = [('version', C.c_int32), ('n_columns', C.c_int32), ('n_states', C.c_int32), ('n_classes', C.c_int32),
                ('n_slots', C.c_int32), ('start_state', C.c_int32), ('reserved', C.c_int32 * 10), ('bias', C.c_void_p),
                ('token_class', C.c_void_p), ('next_state', C.c_void_p), ('slot_open', C.c_void_p), ('slot_close', C.c_void_p)]


class FsmgConstraintState(C.Structure):
    _fields_ = [('state', C.c_void_p), ('open', C.c_void_p), ('dead_ends', C.c_void_p)]


FSMG_BEAM_CONFIG_VERSION = 1


class FsmgBeamConfig(C.Structure):
    _fields_ = [('version', C.c_int32), ('n_groups', C.c_int32), ('beam_width', C.c_int32), ('num', C.c_int32),
                ('primer_len', C.c_int32), ('primer_on_device', C.c_int32), ('reserved', C.c_int32 * 8)]


FSMG_SCORE_CONFIG_VERSION = 1
FSMG_SCORE_PASS_ROWS = 128


class FsmgScoreConfig(C.Structure):
    _fields_ = [('version', C.c_int32), ('n_rows', C.c_int32), ('tokens_on_device', C.c_int32), ('nll_first', C.c_int32),
                ('nll_count', C.c_int32), ('pass_rows', C.c_int32), ('reserved', C.c_int32 * 10)]


FSMG_DSTATE_CONFIG_VERSION = 1


class FsmgDstateConfig(C.Structure):
    _fields_ = [('version', C.c_int32), ('n_rows', C.c_int32), ('history', C.c_int32), ('reserved', C.c_int32 * 9)]


FSMG_CACHE_CONFIG_VERSION = 1
FSMG_CACHE_SCORE_CONFIG_VERSION = 1
FSMG_CACHE_MAX_THETA = 8
FSMG_CACHE_MAX_LAMBDA = 16


class FsmgCacheConfig(C.Structure):
    _fields_ = [('version', C.c_int32), ('n_rows', C.c_int32), ('n_groups', C.c_int32), ('tokens_on_device', C.c_int32),
                ('pass_rows', C.c_int32), ('reserved', C.c_int32 * 11)]


class FsmgCacheScoreConfig(C.Structure):
    _fields_ = [('version', C.c_int32), ('n_rows', C.c_int32), ('tokens_on_device', C.c_int32), ('nll_first', C.c_int32),
                ('nll_count', C.c_int32), ('pass_rows', C.c_int32), ('n_theta', C.c_int32), ('n_lambda', C.c_int32),
                ('thetas', C.c_float * 8), ('lambdas', C.c_float * 16), ('reserved', C.c_int32 * 8)]


FSMG_CACHE_GEN_CONFIG_VERSION = 1
FSMG_CACHE_GEN_CHUNK = 16       # keys per wave of the score kernel of cache-conditioned generation (include/fsmg.h)


class FsmgCacheGenConfig(C.Structure):
    _fields_ = [('version', C.c_int32), ('theta', C.c_float), ('lambda_', C.c_float), ('reserved', C.c_int32 * 13)]


FSMG_CACHE_SELF_CONFIG_VERSION = 1


class FsmgCacheSelfConfig(C.Structure):
    _fields_ = [('version', C.c_int32), ('window', C.c_int32), ('reserved', C.c_int32 * 14)]


DYNEVAL_RULES = {'sgd': 0, 'rms': 1}


class FsmgDynevalConfig(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('rule', C.c_int32), ('seg_len', C.c_int32), ('rows_per_step', C.c_int32),
                ('lr', C.c_float), ('decay', C.c_float), ('eps', C.c_float), ('clip_norm', C.c_float),
                ('adapt_reported', C.c_int32), ('reserved', C.c_int32)]


class FsmgMsgdConfig(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('alpha_init', C.c_float), ('alpha_lr', C.c_float), ('alpha_min', C.c_float),
                ('alpha_max', C.c_float), ('alpha_clip_norm', C.c_float), ('reserved', C.c_int32)]


class FsmgLoptConfig(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('bF_init', C.c_float), ('bI_init', C.c_float), ('gate_scale', C.c_float),
                ('phi_lr', C.c_float), ('phi_clip_norm', C.c_float), ('max_train_steps', C.c_int32), ('reserved', C.c_int32)]


class FsmgDropoutConfig(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('keep_input', C.c_float), ('keep_output', C.c_float), ('variational', C.c_int32),
                ('seed', C.c_uint64)]


class FsmgMamlTasksConfig(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('inner_steps', C.c_int32), ('inner_lr', C.c_float), ('tokens_on_device', C.c_int32),
                ('table_id', C.c_int32), ('use_table_lengths', C.c_int32), ('reserved', C.c_int32 * 2)]


FSMG_STATE_CONFIG_VERSION = 1
FSMG_STATE_PASS_ROWS = 1024


class FsmgStateConfig(C.Structure):
    _fields_ = [('version', C.c_int32), ('tokens_on_device', C.c_int32), ('reserved', C.c_int32 * 6)]


_P = C.c_void_p
_I32P = C.POINTER(C.c_int32)
_F32P = C.POINTER(C.c_float)
# name -> (restype, argtypes); must list every symbol include/fsmg.h declares
SIGNATURES = {
    'fsmg_version': (C.c_int, []),
    'fsmg_last_error': (C.c_char_p, [_P]),
    'fsmg_state_bytes': (C.c_uint64, [C.POINTER(FsmgConfig)]),
    'fsmg_create': (C.c_int, [C.POINTER(FsmgConfig), C.POINTER(_P)]),
    'fsmg_destroy': (C.c_int, [_P]),
    'fsmg_synchronize': (C.c_int, [_P]),
    'fsmg_init_params': (C.c_int, [_P, C.c_uint64]),
    'fsmg_num_params': (C.c_int, [_P]),
    'fsmg_param_info': (C.c_int, [_P, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'fsmg_set_param': (C.c_int, [_P, C.c_char_p, _F32P, C.c_int64]),
    'fsmg_get_param': (C.c_int, [_P, C.c_char_p, _F32P, C.c_int64]),
    'fsmg_set_opt_state': (C.c_int, [_P, C.c_char_p, _F32P, _F32P, C.c_int64]),
    'fsmg_get_opt_state': (C.c_int, [_P, C.c_char_p, _F32P, _F32P, C.c_int64]),
    'fsmg_set_step': (C.c_int, [_P, C.c_int64]),
    'fsmg_get_step': (C.c_int, [_P, C.POINTER(C.c_int64)]),
    'fsmg_get_grad': (C.c_int, [_P, C.c_char_p, _F32P, C.c_int64]),
    'fsmg_train_step': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _F32P]),
    'fsmg_forward_backward': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    'fsmg_grad_buffer': (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int64)]),
    'fsmg_grad_bucket': (C.c_int, [_P, C.c_int32, C.POINTER(_P), C.POINTER(C.c_int64)]),
    'fsmg_stream_wait_bucket': (C.c_int, [_P, _P, C.c_int32]),
    'fsmg_apply_update': (C.c_int, [_P, C.c_float, _F32P]),
    'fsmg_comm_unique_id': (C.c_int, [C.c_char_p]),
    'fsmg_comm_init': (C.c_int, [_P, C.c_char_p, C.c_int32, C.c_int32]),
    'fsmg_comm_attach': (C.c_int, [_P, _P, C.c_int32, C.c_int32]),
    'fsmg_comm_broadcast_state': (C.c_int, [_P, C.c_int32]),
    'fsmg_comm_release': (C.c_int, [_P]),
    'fsmg_upload_table': (C.c_int, [_P, C.c_int32, _P, C.c_int64]),
    'fsmg_forward_backward_indexed': (C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32]),
    'fsmg_train_step_indexed': (C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, _F32P]),
    'fsmg_maml_forward_backward': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32]),
    'fsmg_maml_step': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, _F32P]),
    'fsmg_maml_eval': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, _F32P]),
    'fsmg_maml_forward_backward_indexed': (C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float]),
    'fsmg_maml_step_indexed': (C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, _F32P]),
    'fsmg_maml_forward_backward_masked': (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32]),
    'fsmg_maml_step_masked': (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, _F32P]),
    'fsmg_maml_eval_masked': (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, _F32P]),
    'fsmg_maml_forward_backward_indexed_masked': (C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float]),
    'fsmg_maml_step_indexed_masked': (C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, _F32P]),
    'fsmg_eval_step': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _F32P]),
    'fsmg_eval_batch': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _F32P]),
    'fsmg_train_step_masked': (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _F32P]),
    'fsmg_forward_backward_masked': (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    'fsmg_eval_step_masked': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _F32P]),
    'fsmg_eval_batch_masked': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _F32P]),
    'fsmg_upload_table_lengths': (C.c_int, [_P, C.c_int32, _P, C.c_int64]),
    'fsmg_train_step_indexed_masked': (C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, _F32P]),
    'fsmg_forward_backward_indexed_masked': (C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32]),
    'fsmg_sample': (C.c_int, [_P, C.c_int32, _I32P]),
    'fsmg_generate': (C.c_int, [_P, C.POINTER(FsmgGenConfig), _P, _I32P, _F32P]),
    'fsmg_maml_generate': (C.c_int, [_P, C.POINTER(FsmgGenConfig), _P, C.c_int32, C.c_int32, C.c_float, C.c_int32, _P, _I32P, _F32P]),
    'fsmg_generate_filtered': (C.c_int, [_P, C.POINTER(FsmgGenConfig), C.POINTER(FsmgGenFilters), _P, _I32P, _F32P]),
    'fsmg_maml_generate_filtered': (C.c_int, [_P, C.POINTER(FsmgGenConfig), C.POINTER(FsmgGenFilters), _P, C.c_int32, C.c_int32, C.c_float,
                                              C.c_int32, _P, _I32P, _F32P]),
    'fsmg_maml_generate_filtered_masked': (C.c_int, [_P, C.POINTER(FsmgGenConfig), C.POINTER(FsmgGenFilters), _P, _P, C.c_int32, C.c_int32,
                                                     C.c_float, C.c_int32, _P, _I32P, _F32P]),
    'fsmg_constraint_create': (C.c_int, [_P, C.POINTER(FsmgConstraintConfig), C.POINTER(_P)]),
    'fsmg_constraint_destroy': (C.c_int, [_P, _P]),
    'fsmg_constraint_info': (C.c_int, [_P, _P, C.POINTER(C.c_int64)]),
    'fsmg_generate_constrained': (C.c_int, [_P, C.POINTER(FsmgGenConfig), C.POINTER(FsmgGenFilters), _P, C.POINTER(FsmgConstraintState),
                                            _P, _I32P, _F32P]),
    'fsmg_dstate_generate_constrained': (C.c_int, [_P, _P, C.POINTER(FsmgGenConfig), C.POINTER(FsmgGenFilters), _P,
                                                   C.POINTER(FsmgConstraintState), _I32P, _F32P]),
    'fsmg_maml_generate_constrained': (C.c_int, [_P, C.POINTER(FsmgGenConfig), C.POINTER(FsmgGenFilters), _P, C.POINTER(FsmgConstraintState),
                                                 _P, _P, C.c_int32, C.c_int32, C.c_float, C.c_int32, _P, _I32P, _F32P]),
    'fsmg_beam_search': (C.c_int, [_P, C.POINTER(FsmgBeamConfig), _P, _I32P, _F32P, _F32P]),
    'fsmg_maml_beam_search': (C.c_int, [_P, C.POINTER(FsmgBeamConfig), _P, C.c_int32, C.c_int32, C.c_float, C.c_int32, _P, _I32P, _F32P,
                                        _F32P]),
    'fsmg_maml_beam_search_masked': (C.c_int, [_P, C.POINTER(FsmgBeamConfig), _P, _P, C.c_int32, C.c_int32, C.c_float, C.c_int32, _P, _I32P,
                                               _F32P, _F32P]),
    'fsmg_beam_search_constrained': (C.c_int, [_P, C.POINTER(FsmgBeamConfig), _P, C.POINTER(FsmgConstraintState),
                                               C.POINTER(FsmgConstraintState), _P, _I32P, _F32P, _F32P]),
    'fsmg_dstate_beam_search_constrained': (C.c_int, [_P, _P, C.POINTER(FsmgBeamConfig), _P, C.POINTER(FsmgConstraintState),
                                                      C.POINTER(FsmgConstraintState), _I32P, _F32P, _F32P]),
    'fsmg_maml_beam_search_constrained': (C.c_int, [_P, C.POINTER(FsmgBeamConfig), _P, C.POINTER(FsmgConstraintState),
                                                    C.POINTER(FsmgConstraintState), _P, _P, C.c_int32, C.c_int32, C.c_float, C.c_int32, _P,
                                                    _I32P, _F32P, _F32P]),
    'fsmg_score': (C.c_int, [_P, C.POINTER(FsmgScoreConfig), _P, _F32P, _I32P, _F32P, _I32P, _F32P]),
    'fsmg_maml_score_masked': (C.c_int, [_P, C.POINTER(FsmgScoreConfig), _P, _P, C.c_int32, C.c_int32, C.c_float, C.c_int32, _P, _I32P,
                                         _F32P, _I32P, _F32P, _I32P, _F32P]),
    'fsmg_maml_score': (C.c_int, [_P, C.POINTER(FsmgScoreConfig), _P, C.c_int32, C.c_int32, C.c_float, C.c_int32, _P, _F32P, _I32P,
                                  _F32P, _I32P, _F32P]),
    'fsmg_dstate_create': (C.c_int, [_P, C.POINTER(FsmgDstateConfig), C.POINTER(_P)]),
    'fsmg_dstate_destroy': (C.c_int, [_P, _P]),
    'fsmg_dstate_reset': (C.c_int, [_P, _P]),
    'fsmg_dstate_info': (C.c_int, [_P, _P, C.POINTER(C.c_int64)]),
    'fsmg_dstate_get': (C.c_int, [_P, _P, _F32P, _F32P, _I32P]),
    'fsmg_dstate_set': (C.c_int, [_P, _P, _F32P, _F32P, _I32P, C.c_int64, C.c_int64]),
    'fsmg_dstate_gather': (C.c_int, [_P, _P, _P, _I32P]),
    'fsmg_dstate_feed': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _F32P]),
    'fsmg_dstate_generate': (C.c_int, [_P, _P, C.POINTER(FsmgGenConfig), C.POINTER(FsmgGenFilters), _I32P, _F32P]),
    'fsmg_dstate_beam_search': (C.c_int, [_P, _P, C.POINTER(FsmgBeamConfig), _I32P, _F32P, _F32P]),
    'fsmg_cache_build': (C.c_int, [_P, C.POINTER(FsmgCacheConfig), _P, C.POINTER(_P)]),
    'fsmg_cache_create_from': (C.c_int, [_P, C.c_int32, C.c_int32, _F32P, _I32P, C.POINTER(_P)]),
    'fsmg_cache_get': (C.c_int, [_P, _P, _F32P, _I32P]),
    'fsmg_cache_info': (C.c_int, [_P, _P, C.POINTER(C.c_int64)]),
    'fsmg_cache_destroy': (C.c_int, [_P, _P]),
    'fsmg_cache_attend': (C.c_int, [_P, _P, C.c_int32, _F32P, _I32P, _I32P, _F32P, C.c_int32, _F32P]),
    'fsmg_cache_score': (C.c_int, [_P, _P, C.POINTER(FsmgCacheScoreConfig), _P, _I32P, _F32P, _F32P, _F32P, _F32P]),
    'fsmg_cache_eval_step': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, _F32P]),
    'fsmg_score_masked': (C.c_int, [_P, C.POINTER(FsmgScoreConfig), _P, _I32P, _F32P, _I32P, _F32P, _I32P, _F32P]),
    'fsmg_cache_build_masked': (C.c_int, [_P, C.POINTER(FsmgCacheConfig), _P, _I32P, C.POINTER(_P)]),
    'fsmg_cache_create_from_counts': (C.c_int, [_P, C.c_int32, C.c_int32, _I32P, _F32P, _I32P, C.POINTER(_P)]),
    'fsmg_cache_counts': (C.c_int, [_P, _P, _I32P]),
    'fsmg_cache_score_masked': (C.c_int, [_P, _P, C.POINTER(FsmgCacheScoreConfig), _P, _I32P, _I32P, _F32P, _F32P, _F32P, _F32P]),
    'fsmg_cache_self_score_masked': (C.c_int, [_P, _P, C.POINTER(FsmgCacheScoreConfig), C.POINTER(FsmgCacheSelfConfig), _P, _I32P, _I32P,
                                               _F32P, _F32P, _F32P, _F32P]),
    'fsmg_cache_eval_step_masked': (C.c_int, [_P, _P, _P, _I32P, _I32P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, _F32P]),
    'fsmg_cache_generate': (C.c_int, [_P, _P, C.POINTER(FsmgCacheGenConfig), C.POINTER(FsmgGenConfig), C.POINTER(FsmgGenFilters), _I32P, _P,
                                      _I32P, _F32P]),
    'fsmg_dstate_cache_generate': (C.c_int, [_P, _P, _P, C.POINTER(FsmgCacheGenConfig), C.POINTER(FsmgGenConfig),
                                             C.POINTER(FsmgGenFilters), _I32P, _I32P, _F32P]),
    'fsmg_cache_distribution': (C.c_int, [_P, _P, C.POINTER(FsmgCacheGenConfig), C.c_int32, _F32P, _F32P, _I32P, _F32P, _F32P, _F32P]),
    'fsmg_cache_self_score': (C.c_int, [_P, _P, C.POINTER(FsmgCacheScoreConfig), C.POINTER(FsmgCacheSelfConfig), _P, _I32P, _F32P, _F32P,
                                        _F32P, _F32P]),
    'fsmg_cache_self_attend': (C.c_int, [_P, _P, C.POINTER(FsmgCacheSelfConfig), C.c_int32, C.c_int32, _F32P, _I32P, _I32P, _F32P, C.c_int32,
                                         _F32P]),
    'fsmg_cache_self_generate': (C.c_int, [_P, _P, C.POINTER(FsmgCacheGenConfig), C.POINTER(FsmgCacheSelfConfig), C.POINTER(FsmgGenConfig),
                                           C.POINTER(FsmgGenFilters), _I32P, _P, _I32P, _F32P]),
    'fsmg_cache_self_distribution': (C.c_int, [_P, _P, C.POINTER(FsmgCacheGenConfig), C.POINTER(FsmgCacheSelfConfig), C.c_int32, _F32P, _F32P,
                                               _F32P, _I32P, _I32P, C.c_int32, _I32P, _F32P, _F32P, _F32P]),
    'fsmg_read_losses': (C.c_int, [_P, _F32P, C.c_int32]),
    'fsmg_get_stats': (C.c_int, [_P, C.POINTER(FsmgStats)]),
    'fsmg_debug_read': (C.c_int, [_P, C.c_char_p, _F32P, C.c_int64]),
    'fsmg_debug_dims': (C.c_int, [_P, _I32P]),
    'fsmg_debug_set': (C.c_int, [_P, C.c_char_p, C.c_int64]),
    'fsmg_debug_clock_begin': (C.c_int, [_P, C.c_int32]),
    'fsmg_debug_clock_end': (C.c_int, [_P, _F32P]),
    'fsmg_unigram_create': (C.c_int, [C.c_int32, C.c_int32, C.POINTER(_P)]),
    'fsmg_unigram_destroy': (C.c_int, [_P]),
    'fsmg_unigram_last_error': (C.c_char_p, [_P]),
    'fsmg_unigram_nll': (C.c_int, [_P, _P, C.c_int64, C.c_int32, _F32P]),
    'fsmg_unigram_train': (C.c_int, [_P, _P, C.c_int64, C.c_int32, _F32P]),
    'fsmg_unigram_get_counts': (C.c_int, [_P, _F32P, C.c_int64]),
    'fsmg_unigram_set_counts': (C.c_int, [_P, _F32P, C.c_int64]),
    'fsmg_unigram_argmax': (C.c_int, [_P, _I32P]),
    'fsmg_debug_step_profile': (C.c_int, [_P, C.c_int32, C.POINTER(C.c_uint64), C.c_int64, _I32P, _I32P]),
    'fsmg_timing_enable': (C.c_int, [_P, C.c_int32]),
    'fsmg_timing_select': (C.c_int, [_P, C.c_char_p]),
    'fsmg_timing_read': (C.c_int, [_P, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    'fsmg_timing_reset': (C.c_int, [_P]),
    'fsmg_dyneval_stats_reset': (C.c_int, [_P]),
    'fsmg_dyneval_stats_accumulate': (C.c_int, [_P]),
    'fsmg_dyneval_stats_info': (C.c_int, [_P, C.POINTER(C.c_int64), _F32P]),
    'fsmg_dyneval_stats_get': (C.c_int, [_P, C.c_char_p, _F32P, C.c_int64]),
    'fsmg_dyneval_stats_set': (C.c_int, [_P, C.c_char_p, _F32P, C.c_int64]),
    'fsmg_dyneval_stats_set_count': (C.c_int, [_P, C.c_int64]),
    'fsmg_dyneval_score': (C.c_int, [_P, C.POINTER(FsmgDynevalConfig), _P, _P, C.c_int32, C.c_int32, _F32P, _F32P, _F32P]),
    'fsmg_dyneval_eval_step': (C.c_int, [_P, C.POINTER(FsmgDynevalConfig), _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _F32P]),
    'fsmg_msgd_enable': (C.c_int, [_P, C.POINTER(FsmgMsgdConfig)]),
    'fsmg_msgd_disable': (C.c_int, [_P]),
    'fsmg_msgd_info': (C.c_int, [_P, C.POINTER(C.c_int64)]),
    'fsmg_msgd_fill': (C.c_int, [_P, C.c_float]),
    'fsmg_msgd_get_alpha': (C.c_int, [_P, C.c_char_p, _F32P, C.c_int64]),
    'fsmg_msgd_set_alpha': (C.c_int, [_P, C.c_char_p, _F32P, C.c_int64]),
    'fsmg_msgd_get_opt_state': (C.c_int, [_P, C.c_char_p, _F32P, _F32P, C.c_int64]),
    'fsmg_msgd_set_opt_state': (C.c_int, [_P, C.c_char_p, _F32P, _F32P, C.c_int64]),
    'fsmg_msgd_get_grad': (C.c_int, [_P, C.c_char_p, _F32P, C.c_int64]),
    'fsmg_msgd_grad_buffer': (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int64)]),
    'fsmg_lopt_enable': (C.c_int, [_P, C.POINTER(FsmgLoptConfig)]),
    'fsmg_lopt_disable': (C.c_int, [_P]),
    'fsmg_lopt_info': (C.c_int, [_P, C.POINTER(C.c_int64)]),
    'fsmg_lopt_get_phi': (C.c_int, [_P, _F32P]),
    'fsmg_lopt_set_phi': (C.c_int, [_P, _F32P]),
    'fsmg_lopt_get_opt_state': (C.c_int, [_P, _F32P, _F32P]),
    'fsmg_lopt_set_opt_state': (C.c_int, [_P, _F32P, _F32P]),
    'fsmg_lopt_get_grad': (C.c_int, [_P, _F32P]),
    'fsmg_lopt_grad_buffer': (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int64)]),
    'fsmg_dropout_enable': (C.c_int, [_P, C.POINTER(FsmgDropoutConfig)]),
    'fsmg_dropout_disable': (C.c_int, [_P]),
    'fsmg_dropout_info': (C.c_int, [_P, C.POINTER(C.c_int64)]),
    'fsmg_dropout_set_pass': (C.c_int, [_P, C.c_int64]),
    'fsmg_dropout_mask': (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_uint8)]),
    'fsmg_dyneval_generate': (C.c_int, [_P, C.POINTER(FsmgDynevalConfig), _P, _P, C.c_int32, C.POINTER(FsmgGenConfig),
                                        C.POINTER(FsmgGenFilters), _P, _I32P, _F32P]),
    'fsmg_score_state': (C.c_int, [_P, _P, C.POINTER(FsmgStateConfig), _P, _I32P, _F32P, _I32P, _F32P, _I32P, _F32P]),
    'fsmg_eval_step_state': (C.c_int, [_P, _P, C.POINTER(FsmgStateConfig), _P, _I32P, _F32P, _I32P]),
    'fsmg_forward_backward_state': (C.c_int, [_P, _P, C.POINTER(FsmgStateConfig), _P, _I32P]),
    'fsmg_train_step_state': (C.c_int, [_P, _P, C.POINTER(FsmgStateConfig), _P, _I32P, _F32P]),
    'fsmg_maml_tasks_forward_backward': (C.c_int, [_P, C.POINTER(FsmgMamlTasksConfig), _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32]),
    'fsmg_maml_tasks_step': (C.c_int, [_P, C.POINTER(FsmgMamlTasksConfig), _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _F32P, _F32P]),
    'fsmg_maml_tasks_eval': (C.c_int, [_P, C.POINTER(FsmgMamlTasksConfig), _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _F32P, _F32P]),
}

_lib = None


def library_path():
    return LIB


def load_library():
    """dlopen the in-tree libfsmg.so; raises (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB):
            raise FsmgError(-2, 'libfsmg.so not built (%s); run `python -c "import __graft_entry__ as g; g.build()"` '
                                'or `make -C few-shot-music-generation_amd/csrc` -- there is no CPU fallback' % LIB)
        # PyTorch-ROCm ships its own libamdhip64; whichever HIP runtime is loaded first serves the whole
        # process.  Load torch's first (when torch is installed) so that torch.cuda / RCCL and libfsmg share
        # one runtime regardless of import order -- the reverse order leaves torch with "No HIP GPUs".
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = C.CDLL(LIB)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def _f32p(a):
    return a.ctypes.data_as(_F32P)


def _tok_ptr(tokens):
    """host numpy int32 array or a raw device address (int) -> (void*, on_device, keepalive)"""
    if isinstance(tokens, (int, np.integer)):
        return C.c_void_p(int(tokens)), 1, None
    a = np.ascontiguousarray(tokens, dtype=np.int32)
    return C.c_void_p(a.ctypes.data), 0, a


class DecodeState(object):
    """A decode state of an FsmgModel (include/fsmg.h fsmg_dstate_*): h and c of every layer, the pending token and the last
    `history` context tokens of `rows` decode rows, resident on the device.  Made by FsmgModel.new_state; FsmgModel.feed and the
    state= keyword of FsmgModel.generate / beam_search start from it (feed and generate leave it advanced)."""

    def __init__(self, model, rows, history):
        self._model = model
        self.rows, self.history = int(rows), int(history)
        c = FsmgDstateConfig(version=FSMG_DSTATE_CONFIG_VERSION, n_rows=self.rows, history=self.history)
        st = _P()
        model._ck(model._lib.fsmg_dstate_create(model._h, C.byref(c), C.byref(st)))
        self._st = st

    def close(self):
        # (a state whose model is closed already went with it: fsmg_destroy frees what is left)
        if getattr(self, '_st', None) and getattr(self._model, '_h', None):
            self._model._lib.fsmg_dstate_destroy(self._model._h, self._st)
        self._st = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, fn, *args):
        if not getattr(self, '_st', None):
            raise FsmgError(-1, 'the decode state is closed')
        self._model._ck(fn(self._model._h, self._st, *args))

    def reset(self):
        """back to the fresh state: zero h and c, no context, the start word pending"""
        self._call(self._model._lib.fsmg_dstate_reset)

    def info(self):
        out = (C.c_int64 * 4)()
        self._call(self._model._lib.fsmg_dstate_info, out)
        return dict(rows=int(out[0]), history=int(out[1]), n_ctx=int(out[2]), n_gen=int(out[3]))

    def _layers(self):
        return int(self._model.cfg.n_layers), int(self._model.cfg.hidden_size)

    def get(self):
        """-> dict: 'h', 'c' float32 [L, rows, H], 'ctx' int32 [rows, min(n_ctx, history)] (oldest first), 'n_ctx', 'n_gen'"""
        L, H = self._layers()
        info = self.info()
        hh, cc = np.empty((L, self.rows, H), np.float32), np.empty((L, self.rows, H), np.float32)
        ctx = np.empty((self.rows, min(info['n_ctx'], self.history)), np.int32)
        self._call(self._model._lib.fsmg_dstate_get, _f32p(hh), _f32p(cc), ctx.ctypes.data_as(_I32P))
        return dict(h=hh, c=cc, ctx=ctx, n_ctx=info['n_ctx'], n_gen=info['n_gen'])

    def set(self, h, c, ctx=None, n_ctx=0, n_gen=0):
        """the reverse of get: h, c [L, rows, H]; ctx [rows, min(n_ctx, history)] (None when n_ctx is 0)"""
        L, H = self._layers()
        hh, cc = np.ascontiguousarray(h, dtype=np.float32), np.ascontiguousarray(c, dtype=np.float32)
        if hh.shape != (L, self.rows, H) or cc.shape != (L, self.rows, H):
            raise ValueError('h and c must be [%d, %d, %d], got %r and %r' % (L, self.rows, H, hh.shape, cc.shape))
        keep = min(int(n_ctx), self.history)
        a = None
        if keep > 0:
            a = np.ascontiguousarray(ctx, dtype=np.int32)
            if a.shape != (self.rows, keep):
                raise ValueError('ctx must be [%d, %d], got %r' % (self.rows, keep, a.shape))
        self._call(self._model._lib.fsmg_dstate_set, _f32p(hh), _f32p(cc), a.ctypes.data_as(_I32P) if a is not None else None,
                   int(n_ctx), int(n_gen))

    def gather(self, src, rows):
        """this state's row i = row rows[i] of src (another state of the same model and history); the counters are copied"""
        idx = np.ascontiguousarray(rows, dtype=np.int32)
        if idx.shape != (self.rows,):
            raise ValueError('rows must be [%d] indices, got %r' % (self.rows, idx.shape))
        if not isinstance(src, DecodeState) or not getattr(src, '_st', None):
            raise ValueError('src must be an open DecodeState')
        self._call(self._model._lib.fsmg_dstate_gather, src._st, idx.ctypes.data_as(_I32P))


class DeviceConstraint(object):
    """A constraint resident on the device (include/fsmg.h fsmg_constraint_*): the tables of a data.constraints.Constraints
    (or any object with its attributes) uploaded once for one FsmgModel.  Made by FsmgModel.new_constraint; the constraints=
    keyword of FsmgModel.generate / maml_generate takes one (or the host object, which is uploaded and cached on the model)."""

    def __init__(self, model, con):
        self._model = model
        keep = []

        def ptr(a, dtype):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dtype)
            keep.append(a)
            return C.c_void_p(a.ctypes.data)
        nxt = getattr(con, 'next_state', None)
        c = FsmgConstraintConfig(version=FSMG_CONSTRAINT_CONFIG_VERSION, n_columns=int(con.n_columns),
                                 n_states=0 if nxt is None else int(np.asarray(nxt).shape[0]),
                                 n_classes=0 if nxt is None else int(np.asarray(nxt).shape[1]), n_slots=int(con.n_slots),
                                 start_state=int(con.start_state), bias=ptr(con.bias, np.float32),
                                 token_class=ptr(con.token_class, np.int32), next_state=ptr(nxt, np.int32),
                                 slot_open=ptr(con.slot_open, np.int32), slot_close=ptr(con.slot_close, np.int32))
        h = _P()
        model._ck(model._lib.fsmg_constraint_create(model._h, C.byref(c), C.byref(h)))
        self._con = h
        out = (C.c_int64 * 4)()
        model._ck(model._lib.fsmg_constraint_info(model._h, h, out))
        self.n_columns, self.n_states, self.n_classes, self.n_slots = (int(x) for x in out)
        self.n_words = (self.n_slots + 31) // 32
        self.start_state = int(con.start_state)

    def close(self):
        # (a constraint whose model is closed already went with it: fsmg_destroy frees what is left)
        if getattr(self, '_con', None) and getattr(self._model, '_h', None):
            self._model._lib.fsmg_constraint_destroy(self._model._h, self._con)
        self._con = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FsmgCache(object):
    """A support-set cache of an FsmgModel (include/fsmg.h fsmg_cache_*): `groups` groups (one per artist) of `entries` (key, value)
    pairs each, resident on the device -- a key is a top-layer hidden state, a value the token that followed it.  Made by
    FsmgModel.cache_build / cache_from; FsmgModel.cache_attend / cache_score read it.  A cache is data: it stays valid, and stale,
    when the parameters change."""

    def __init__(self, model, handle):
        self._model = model
        self._c = handle
        i = self.info()
        self.groups, self.entries, self.hidden = i['groups'], i['entries'], i['hidden']

    def close(self):
        # (a cache whose model is closed already went with it: fsmg_destroy frees what is left)
        if getattr(self, '_c', None) and getattr(self._model, '_h', None):
            self._model._lib.fsmg_cache_destroy(self._model._h, self._c)
        self._c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ptr(self):
        if not getattr(self, '_c', None):
            raise FsmgError(-1, 'the cache is closed')
        return self._c

    def _call(self, fn, *args):
        self._model._ck(fn(self._model._h, self._ptr(), *args))

    def info(self):
        out = (C.c_int64 * 4)()
        self._call(self._model._lib.fsmg_cache_info, out)
        return dict(groups=int(out[0]), entries=int(out[1]), hidden=int(out[2]), bytes=int(out[3]))

    def get(self):
        """-> (keys float32 [groups, entries, H], values int32 [groups, entries])"""
        keys = np.empty((self.groups, self.entries, self.hidden), np.float32)
        vals = np.empty((self.groups, self.entries), np.int32)
        self._call(self._model._lib.fsmg_cache_get, _f32p(keys), vals.ctypes.data_as(_I32P))
        return keys, vals

    def counts(self):
        """-> int32 [groups]: the entries each group holds -- `entries` for every group of a uniform cache; a ragged one (cache_build
        with lengths, cache_from with counts) holds fewer, and the slots behind them read back as zeros"""
        out = np.empty(self.groups, np.int32)
        self._call(self._model._lib.fsmg_cache_counts, out.ctypes.data_as(_I32P))
        return out


class FsmgModel(object):
    """One model handle == one LSTM language model resident on one MI355X."""

    def __init__(self, config, device=0, stream=None, state_arena=None, state_arena_bytes=0,
                 max_sequences=0, clip_norm_mode='tf1_slices', use_graph=True, gemm=None, schedule=None, recurrence=None,
                 dp_split_backward=None):
        self._lib = load_library()
        # schedule / arithmetic knobs: explicit arguments, else optional keys of the model config, else the library's choice
        gemm = gemm or config.get('gemm', 'auto')
        schedule = schedule or config.get('schedule', 'auto')
        recurrence = recurrence or config.get('recurrence', 'auto')
        if dp_split_backward is None:
            dp_split_backward = config.get('dp_split_backward', False)
        self.cfg = FsmgConfig(
            input_size=int(config['input_size']), max_len=int(config['max_len']),
            embedding_size=int(config['embedding_size']), hidden_size=int(config['hidden_size']),
            n_layers=int(config['n_layers']), lr=float(config['lr']),
            max_grad_norm=float(config['max_grad_norm']), n_decay=float(config['n_decay']),
            clip_norm_mode=CLIP_MODES[clip_norm_mode], device=int(device), max_sequences=int(max_sequences),
            use_graph=int(bool(use_graph)), stream=stream, state_arena=state_arena,
            state_arena_bytes=int(state_arena_bytes), config_version=FSMG_CONFIG_VERSION, gemm=GEMM_KINDS[gemm],
            schedule=SCHEDULES[schedule], recurrence=RECURRENCES[recurrence], dp_split_backward=(2 if dp_split_backward == 2 and dp_split_backward is not True else int(bool(dp_split_backward))))
        self.max_len = int(config['max_len'])
        handle = _P()
        rc = self._lib.fsmg_create(C.byref(self.cfg), C.byref(handle))
        if rc != 0:
            raise FsmgError(rc, self._lib.fsmg_last_error(None).decode())
        self._h = handle
        self.param_shapes = {}
        for i in range(self._lib.fsmg_num_params(self._h)):
            name = C.create_string_buffer(64)
            rows, cols = C.c_int64(), C.c_int64()
            self._ck(self._lib.fsmg_param_info(self._h, i, name, 64, C.byref(rows), C.byref(cols)))
            self.param_shapes[name.value.decode()] = (rows.value, cols.value)

    @staticmethod
    def state_bytes(config):
        lib = load_library()
        cfg = FsmgConfig(input_size=int(config['input_size']), max_len=int(config['max_len']),
                         embedding_size=int(config['embedding_size']), hidden_size=int(config['hidden_size']),
                         n_layers=int(config['n_layers']), lr=1.0, max_grad_norm=1.0, n_decay=1.0,
                         config_version=FSMG_CONFIG_VERSION)
        return int(lib.fsmg_state_bytes(C.byref(cfg)))

    def _ck(self, rc):
        if rc != 0:
            raise FsmgError(rc, self._lib.fsmg_last_error(self._h).decode())

    def close(self):
        if getattr(self, '_h', None):
            self._lib.fsmg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- parameters -------------------------------------------------------------------------
    def _shape(self, name):
        if name not in self.param_shapes:
            raise FsmgError(-5, "unknown parameter '%s'" % name)
        rows, cols = self.param_shapes[name]
        vector = name.startswith('bias_') or name == 'softmax_b'        # cols == 1 alone cannot tell a vector from an [n, 1] matrix (E = 1)
        return (rows,) if vector else (rows, cols)

    def init_params(self, seed):
        self._ck(self._lib.fsmg_init_params(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF))

    def set_param(self, name, value):
        a = np.ascontiguousarray(value, dtype=np.float32)
        self._ck(self._lib.fsmg_set_param(self._h, name.encode(), _f32p(a), a.size))

    def get_param(self, name):
        out = np.empty(self._shape(name), np.float32)
        self._ck(self._lib.fsmg_get_param(self._h, name.encode(), _f32p(out), out.size))
        return out

    def set_params(self, params):
        for k, v in params.items():
            self.set_param(k, v)

    def get_params(self):
        return {k: self.get_param(k) for k in self.param_shapes}

    def get_grad(self, name):
        out = np.empty(self._shape(name), np.float32)
        self._ck(self._lib.fsmg_get_grad(self._h, name.encode(), _f32p(out), out.size))
        return out

    def get_opt_state(self, name):
        m = np.empty(self._shape(name), np.float32)
        v = np.empty(self._shape(name), np.float32)
        self._ck(self._lib.fsmg_get_opt_state(self._h, name.encode(), _f32p(m), _f32p(v), m.size))
        return m, v

    def set_opt_state(self, name, m, v):
        m = np.ascontiguousarray(m, dtype=np.float32)
        v = np.ascontiguousarray(v, dtype=np.float32)
        self._ck(self._lib.fsmg_set_opt_state(self._h, name.encode(), _f32p(m), _f32p(v), m.size))

    @property
    def step(self):
        s = C.c_int64()
        self._ck(self._lib.fsmg_get_step(self._h, C.byref(s)))
        return s.value

    @step.setter
    def step(self, value):
        self._ck(self._lib.fsmg_set_step(self._h, int(value)))

    # -- hot path -----------------------------------------------------------------------------
    def _episode_shape(self, support, query, shape):
        if shape is not None:
            return shape
        n, k, t = support.shape
        n2, q, t2 = query.shape
        if n != n2 or t != self.max_len or t2 != self.max_len:
            raise ValueError('support %r / query %r do not match max_len=%d' % (support.shape, query.shape, self.max_len))
        return n, k, q

    def train_step(self, support, query, shape=None, want_loss=True):
        """support [N,K,T], query [N,Q,T] int32 (numpy) -- or raw device addresses with shape=(N,K,Q)."""
        n, k, q = self._episode_shape(support, query, shape)
        sp, dev, _k1 = _tok_ptr(support)
        qp, _, _k2 = _tok_ptr(query)
        loss = C.c_float()
        self._ck(self._lib.fsmg_train_step(self._h, sp, qp, n, k, q, dev, C.byref(loss) if want_loss else None))
        return loss.value if want_loss else None

    def forward_backward(self, support, query, shape=None):
        n, k, q = self._episode_shape(support, query, shape)
        sp, dev, _k1 = _tok_ptr(support)
        qp, _, _k2 = _tok_ptr(query)
        self._ck(self._lib.fsmg_forward_backward(self._h, sp, qp, n, k, q, dev))

    # -- padding-masked forms (include/fsmg.h "per-song lengths"): position t of row b is scored iff t < len[b] ---------------
    @staticmethod
    def _len_ptr(lengths, count, on_device):
        """lengths of `count` sequences: a host int32 array, or a raw device address when the tokens are device pointers"""
        if isinstance(lengths, (int, np.integer)):
            if not on_device:
                raise ValueError('device lengths go with device tokens (one flag covers both)')
            return C.c_void_p(int(lengths)), None
        if on_device:
            raise ValueError('device tokens need device lengths (one flag covers both)')
        if lengths is None:
            raise ValueError('a masked call needs lengths')
        a = np.ascontiguousarray(lengths, dtype=np.int32).reshape(-1)
        if a.size != count:
            raise ValueError('%d lengths for %d sequences' % (a.size, count))
        return C.c_void_p(a.ctypes.data), a

    def train_step_masked(self, support, query, support_len, query_len, shape=None, want_loss=True):
        """train_step with support_len [N,K] / query_len [N,Q] int32 (host arrays, or device addresses with device tokens)"""
        n, k, q = self._episode_shape(support, query, shape)
        sp, dev, _k1 = _tok_ptr(support)
        qp, _, _k2 = _tok_ptr(query)
        sl, _k3 = self._len_ptr(support_len, n * k, dev)
        ql, _k4 = self._len_ptr(query_len, n * q, dev)
        loss = C.c_float()
        self._ck(self._lib.fsmg_train_step_masked(self._h, sp, qp, sl, ql, n, k, q, dev, C.byref(loss) if want_loss else None))
        return loss.value if want_loss else None

    def forward_backward_masked(self, support, query, support_len, query_len, shape=None):
        n, k, q = self._episode_shape(support, query, shape)
        sp, dev, _k1 = _tok_ptr(support)
        qp, _, _k2 = _tok_ptr(query)
        sl, _k3 = self._len_ptr(support_len, n * k, dev)
        ql, _k4 = self._len_ptr(query_len, n * q, dev)
        self._ck(self._lib.fsmg_forward_backward_masked(self._h, sp, qp, sl, ql, n, k, q, dev))

    def eval_step_masked(self, query, query_len, shape=None):
        if shape is None:
            n, q, t = query.shape
            if t != self.max_len:
                raise ValueError('query %r does not match max_len=%d' % (query.shape, self.max_len))
        else:
            n, q = shape
        qp, dev, _k = _tok_ptr(query)
        ql, _k2 = self._len_ptr(query_len, n * q, dev)
        nll = C.c_float()
        self._ck(self._lib.fsmg_eval_step_masked(self._h, qp, ql, n, q, dev, C.byref(nll)))
        return nll.value

    def eval_batch_masked(self, queries, query_len, shape=None):
        """queries [n_episodes,N,Q,T], query_len [n_episodes,N,Q] -> float32 [n_episodes], each over its own n_valid"""
        if shape is None:
            ne, n, q, t = queries.shape
            if t != self.max_len:
                raise ValueError('queries %r do not match max_len=%d' % (queries.shape, self.max_len))
        else:
            ne, n, q = shape
        qp, dev, _k = _tok_ptr(queries)
        ql, _k2 = self._len_ptr(query_len, ne * n * q, dev)
        out = np.empty(ne, np.float32)
        self._ck(self._lib.fsmg_eval_batch_masked(self._h, qp, ql, ne, n, q, dev, _f32p(out)))
        return out

    def forward_backward_indexed_masked(self, table_id, support_idx, query_idx):
        s, q = self._idx(support_idx, query_idx)
        self._ck(self._lib.fsmg_forward_backward_indexed_masked(self._h, int(table_id), C.c_void_p(s.ctypes.data), C.c_void_p(q.ctypes.data),
                                                                s.shape[0], s.shape[1], q.shape[1]))

    def train_step_indexed_masked(self, table_id, support_idx, query_idx, want_loss=True):
        s, q = self._idx(support_idx, query_idx)
        loss = C.c_float()
        self._ck(self._lib.fsmg_train_step_indexed_masked(self._h, int(table_id), C.c_void_p(s.ctypes.data), C.c_void_p(q.ctypes.data),
                                                          s.shape[0], s.shape[1], q.shape[1], C.byref(loss) if want_loss else None))
        return loss.value if want_loss else None

    def grad_buffer(self):
        ptr, count = _P(), C.c_int64()
        self._ck(self._lib.fsmg_grad_buffer(self._h, C.byref(ptr), C.byref(count)))
        return ptr.value, count.value

    def grad_bucket(self, bucket):
        ptr, count = _P(), C.c_int64()
        self._ck(self._lib.fsmg_grad_bucket(self._h, int(bucket), C.byref(ptr), C.byref(count)))
        return ptr.value, count.value

    def stream_wait_bucket(self, stream_handle, bucket):
        self._ck(self._lib.fsmg_stream_wait_bucket(self._h, C.c_void_p(stream_handle), int(bucket)))

    def apply_update(self, grad_scale=1.0, want_loss=True):
        loss = C.c_float()
        self._ck(self._lib.fsmg_apply_update(self._h, float(grad_scale), C.byref(loss) if want_loss else None))
        return loss.value if want_loss else None

    # -- gradient exchange inside the library (RCCL) ---------------------------------------------------
    @staticmethod
    def comm_unique_id():
        '''rank 0: 128 opaque bytes to hand to every rank (ncclGetUniqueId)'''
        lib = load_library()
        buf = C.create_string_buffer(128)
        rc = lib.fsmg_comm_unique_id(buf)
        if rc != 0:
            raise FsmgError(rc, lib.fsmg_last_error(None).decode())
        return buf.raw

    def comm_init(self, unique_id, world_size, rank):
        '''collective: every rank of the job calls it with the id rank 0 made; from then on train_step / train_step_indexed /
        maml_step exchange the gradients themselves (grad_scale 1 / world_size)'''
        self._ck(self._lib.fsmg_comm_init(self._h, C.c_char_p(bytes(unique_id)), int(world_size), int(rank)))

    def comm_broadcast_state(self, root=0):
        self._ck(self._lib.fsmg_comm_broadcast_state(self._h, int(root)))

    def comm_release(self):
        self._ck(self._lib.fsmg_comm_release(self._h))

    # -- device-resident episode table ----------------------------------------------------------------
    def upload_table(self, table_id, table, lengths=None):
        """lengths: int32 [n_songs], the songs' lengths for the masked indexed calls (None: the table has none)"""
        a = np.ascontiguousarray(table, dtype=np.int32)
        if a.ndim != 2 or a.shape[1] != self.max_len:
            raise ValueError('token table %r does not match max_len=%d' % (a.shape, self.max_len))
        if lengths is not None:
            ln = np.ascontiguousarray(lengths, dtype=np.int32)
            if ln.shape != (a.shape[0],):
                raise ValueError('lengths %r do not match the %d songs of the table' % (ln.shape, a.shape[0]))
        self._ck(self._lib.fsmg_upload_table(self._h, int(table_id), C.c_void_p(a.ctypes.data), a.shape[0]))
        if lengths is not None:
            self._ck(self._lib.fsmg_upload_table_lengths(self._h, int(table_id), C.c_void_p(ln.ctypes.data), ln.shape[0]))

    @staticmethod
    def _idx(support_idx, query_idx):
        s = np.ascontiguousarray(support_idx, dtype=np.int32)
        q = np.ascontiguousarray(query_idx, dtype=np.int32)
        if s.ndim != 2 or q.ndim != 2 or s.shape[0] != q.shape[0]:
            raise ValueError('index arrays must be [N, K] and [N, Q]')
        return s, q

    def forward_backward_indexed(self, table_id, support_idx, query_idx):
        s, q = self._idx(support_idx, query_idx)
        self._ck(self._lib.fsmg_forward_backward_indexed(self._h, int(table_id), C.c_void_p(s.ctypes.data), C.c_void_p(q.ctypes.data),
                                                         s.shape[0], s.shape[1], q.shape[1]))

    def train_step_indexed(self, table_id, support_idx, query_idx, want_loss=True):
        s, q = self._idx(support_idx, query_idx)
        loss = C.c_float()
        self._ck(self._lib.fsmg_train_step_indexed(self._h, int(table_id), C.c_void_p(s.ctypes.data), C.c_void_p(q.ctypes.data),
                                                   s.shape[0], s.shape[1], q.shape[1], C.byref(loss) if want_loss else None))
        return loss.value if want_loss else None

    # -- cfg-E: MAML-style inner / outer loop ------------------------------------------------------
    def maml_forward_backward(self, support, query, inner_steps, inner_lr, shape=None):
        n, k, q = self._episode_shape(support, query, shape)
        sp, dev, _k1 = _tok_ptr(support)
        qp, _, _k2 = _tok_ptr(query)
        self._ck(self._lib.fsmg_maml_forward_backward(self._h, sp, qp, n, k, q, int(inner_steps), float(inner_lr), dev))

    def maml_step(self, support, query, inner_steps, inner_lr, shape=None, want_loss=True):
        n, k, q = self._episode_shape(support, query, shape)
        sp, dev, _k1 = _tok_ptr(support)
        qp, _, _k2 = _tok_ptr(query)
        loss = C.c_float()
        self._ck(self._lib.fsmg_maml_step(self._h, sp, qp, n, k, q, int(inner_steps), float(inner_lr), dev,
                                          C.byref(loss) if want_loss else None))
        return loss.value if want_loss else None

    def maml_forward_backward_indexed(self, table_id, support_idx, query_idx, inner_steps, inner_lr):
        s, q = self._idx(support_idx, query_idx)
        self._ck(self._lib.fsmg_maml_forward_backward_indexed(self._h, int(table_id), C.c_void_p(s.ctypes.data), C.c_void_p(q.ctypes.data),
                                                              s.shape[0], s.shape[1], q.shape[1], int(inner_steps), float(inner_lr)))

    def maml_step_indexed(self, table_id, support_idx, query_idx, inner_steps, inner_lr, want_loss=True):
        s, q = self._idx(support_idx, query_idx)
        loss = C.c_float()
        self._ck(self._lib.fsmg_maml_step_indexed(self._h, int(table_id), C.c_void_p(s.ctypes.data), C.c_void_p(q.ctypes.data),
                                                  s.shape[0], s.shape[1], q.shape[1], int(inner_steps), float(inner_lr),
                                                  C.byref(loss) if want_loss else None))
        return loss.value if want_loss else None

    def maml_eval(self, support, query, inner_steps, inner_lr, shape=None):
        n, k, q = self._episode_shape(support, query, shape)
        sp, dev, _k1 = _tok_ptr(support)
        qp, _, _k2 = _tok_ptr(query)
        nll = C.c_float()
        self._ck(self._lib.fsmg_maml_eval(self._h, sp, qp, n, k, q, int(inner_steps), float(inner_lr), dev, C.byref(nll)))
        return nll.value

    # -- cfg-E with per-song lengths (include/fsmg.h "cfg-E with per-song lengths") -----------
    def _maml_masked_args(self, support, query, support_len, query_len, shape):
        n, k, q = self._episode_shape(support, query, shape)
        sp, dev, k1 = _tok_ptr(support)
        qp, _, k2 = _tok_ptr(query)
        sl, k3 = self._len_ptr(support_len, n * k, dev)
        ql, k4 = self._len_ptr(query_len, n * q, dev)
        return (sp, qp, sl, ql, n, k, q), dev, (k1, k2, k3, k4)

    def maml_forward_backward_masked(self, support, query, support_len, query_len, inner_steps, inner_lr, shape=None):
        """maml_forward_backward with support_len [N,K] / query_len [N,Q] int32 (host arrays, or device addresses with device tokens)"""
        a, dev, _keep = self._maml_masked_args(support, query, support_len, query_len, shape)
        self._ck(self._lib.fsmg_maml_forward_backward_masked(self._h, *a, int(inner_steps), float(inner_lr), dev))

    def maml_step_masked(self, support, query, support_len, query_len, inner_steps, inner_lr, shape=None, want_loss=True):
        a, dev, _keep = self._maml_masked_args(support, query, support_len, query_len, shape)
        loss = C.c_float()
        self._ck(self._lib.fsmg_maml_step_masked(self._h, *a, int(inner_steps), float(inner_lr), dev, C.byref(loss) if want_loss else None))
        return loss.value if want_loss else None

    def maml_eval_masked(self, support, query, support_len, query_len, inner_steps, inner_lr, shape=None):
        a, dev, _keep = self._maml_masked_args(support, query, support_len, query_len, shape)
        nll = C.c_float()
        self._ck(self._lib.fsmg_maml_eval_masked(self._h, *a, int(inner_steps), float(inner_lr), dev, C.byref(nll)))
        return nll.value

    def maml_forward_backward_indexed_masked(self, table_id, support_idx, query_idx, inner_steps, inner_lr):
        """the rows' lengths come from the table's own (upload_table(..., lengths=))"""
        s, q = self._idx(support_idx, query_idx)
        self._ck(self._lib.fsmg_maml_forward_backward_indexed_masked(self._h, int(table_id), C.c_void_p(s.ctypes.data), C.c_void_p(q.ctypes.data),
                                                                     s.shape[0], s.shape[1], q.shape[1], int(inner_steps), float(inner_lr)))

    def maml_step_indexed_masked(self, table_id, support_idx, query_idx, inner_steps, inner_lr, want_loss=True):
        s, q = self._idx(support_idx, query_idx)
        loss = C.c_float()
        self._ck(self._lib.fsmg_maml_step_indexed_masked(self._h, int(table_id), C.c_void_p(s.ctypes.data), C.c_void_p(q.ctypes.data),
                                                         s.shape[0], s.shape[1], q.shape[1], int(inner_steps), float(inner_lr),
                                                         C.byref(loss) if want_loss else None))
        return loss.value if want_loss else None

    # -- per-artist MAML (include/fsmg.h "per-artist MAML"): one adaptation per artist -----------
    def _maml_tasks_args(self, support, query, inner_steps, inner_lr, support_len, query_len, table, table_lengths, shape):
        """(config, support, query, support_len, query_len, N, K, Q) of a tasks call and what must stay alive behind it.
        table=None: support [N,K,T] / query [N,Q,T] tokens (or device addresses with shape=), lengths optional and together;
        table=id: support [N,K] / query [N,Q] row indices into that table, table_lengths says whether its lengths mask the passes"""
        cfg = FsmgMamlTasksConfig()
        cfg.struct_size = C.sizeof(FsmgMamlTasksConfig)
        cfg.inner_steps, cfg.inner_lr, cfg.table_id, cfg.use_table_lengths = int(inner_steps), float(inner_lr), -1, 0
        if table is not None:
            if support_len is not None or query_len is not None:
                raise ValueError('a table call takes the table\'s lengths (table_lengths=True), not length arrays')
            s, q = self._idx(support, query)
            cfg.table_id, cfg.use_table_lengths = int(table), 1 if table_lengths else 0
            return (cfg, C.c_void_p(s.ctypes.data), C.c_void_p(q.ctypes.data), None, None, s.shape[0], s.shape[1], q.shape[1]), (s, q)
        if table_lengths:
            raise ValueError('table_lengths needs table=')
        if (support_len is None) != (query_len is None):
            raise ValueError('support_len and query_len go together')
        n, k, q = self._episode_shape(support, query, shape)
        sp, dev, k1 = _tok_ptr(support)
        qp, _, k2 = _tok_ptr(query)
        cfg.tokens_on_device = dev
        sl = ql = k3 = k4 = None
        if support_len is not None:
            sl, k3 = self._len_ptr(support_len, n * k, dev)
            ql, k4 = self._len_ptr(query_len, n * q, dev)
        return (cfg, sp, qp, sl, ql, n, k, q), (k1, k2, k3, k4)

    def maml_tasks_forward_backward(self, support, query, inner_steps, inner_lr, support_len=None, query_len=None, table=None,
                                    table_lengths=False, shape=None):
        a, _keep = self._maml_tasks_args(support, query, inner_steps, inner_lr, support_len, query_len, table, table_lengths, shape)
        self._ck(self._lib.fsmg_maml_tasks_forward_backward(self._h, C.byref(a[0]), *a[1:]))

    def maml_tasks_step(self, support, query, inner_steps, inner_lr, support_len=None, query_len=None, table=None, table_lengths=False,
                        shape=None, want_loss=True, task_loss=False):
        """the mean of the per-artist query losses (None without want_loss); task_loss=True: (loss, [N] float32 array of L_n)"""
        a, _keep = self._maml_tasks_args(support, query, inner_steps, inner_lr, support_len, query_len, table, table_lengths, shape)
        loss = C.c_float()
        per = np.empty(a[5], dtype=np.float32) if task_loss else None
        self._ck(self._lib.fsmg_maml_tasks_step(self._h, C.byref(a[0]), *a[1:], C.byref(loss) if want_loss else None,
                                                _f32p(per) if task_loss else None))
        out = loss.value if want_loss else None
        return (out, per) if task_loss else out

    def maml_tasks_eval(self, support, query, inner_steps, inner_lr, support_len=None, query_len=None, table=None, table_lengths=False,
                        shape=None, task_nll=False):
        """the mean over the artists of the query NLL at that artist's theta'; task_nll=True: (nll, [N] float32 array)"""
        a, _keep = self._maml_tasks_args(support, query, inner_steps, inner_lr, support_len, query_len, table, table_lengths, shape)
        nll = C.c_float()
        per = np.empty(a[5], dtype=np.float32) if task_nll else None
        self._ck(self._lib.fsmg_maml_tasks_eval(self._h, C.byref(a[0]), *a[1:], C.byref(nll), _f32p(per) if task_nll else None))
        return (nll.value, per) if task_nll else nll.value

    def eval_step(self, query, shape=None):
        if shape is None:
            n, q, t = query.shape
            if t != self.max_len:
                raise ValueError('query %r does not match max_len=%d' % (query.shape, self.max_len))
        else:
            n, q = shape
        qp, dev, _k = _tok_ptr(query)
        nll = C.c_float()
        self._ck(self._lib.fsmg_eval_step(self._h, qp, n, q, dev, C.byref(nll)))
        return nll.value

    def eval_batch(self, queries, shape=None):
        """queries [n_episodes,N,Q,T] -> float32 [n_episodes]"""
        if shape is None:
            ne, n, q, t = queries.shape
            if t != self.max_len:
                raise ValueError('queries %r do not match max_len=%d' % (queries.shape, self.max_len))
        else:
            ne, n, q = shape
        qp, dev, _k = _tok_ptr(queries)
        out = np.empty(ne, np.float32)
        self._ck(self._lib.fsmg_eval_batch(self._h, qp, ne, n, q, dev, _f32p(out)))
        return out

    def sample(self, num):
        out = np.empty(max(int(num), 1), np.int32)
        self._ck(self._lib.fsmg_sample(self._h, int(num), out.ctypes.data_as(_I32P)))
        return [int(t) for t in out[:int(num)]]

    # -- batched on-device generation (include/fsmg.h fsmg_generate) ---------------------------------------
    @staticmethod
    def gen_config(n_seq, num, temperature=1.0, top_k=0, seed=0, primer_len=0, primer_on_device=0):
        return FsmgGenConfig(version=FSMG_GEN_CONFIG_VERSION, n_seq=int(n_seq), num=int(num), primer_len=int(primer_len),
                             temperature=float(temperature), top_k=int(top_k), seed=int(seed) & 0xFFFFFFFFFFFFFFFF,
                             primer_on_device=int(primer_on_device))

    @staticmethod
    def _primer(primer, rows, what):
        """primer [rows, P] (or one [P] row for all), or (device address, P) -> (P, on_device, pointer, keepalive)"""
        if primer is None:
            return 0, 0, None, None
        if isinstance(primer, tuple):                 # (device address, primer_len)
            return int(primer[1]), 1, C.c_void_p(int(primer[0])), None
        a = np.ascontiguousarray(primer, dtype=np.int32)
        if a.ndim == 1:
            a = np.ascontiguousarray(np.broadcast_to(a, (int(rows), a.size)))
        if a.ndim != 2 or a.shape[0] != int(rows):
            raise ValueError('primer must be [%s, P] (or one [P] row for every %s), got %r' % (what[0], what[1], a.shape))
        return a.shape[1], 0, C.c_void_p(a.ctypes.data), a

    def _support(self, support, n_support_rows):
        """support [rows, max_len] (numpy), or a device address with n_support_rows -> (pointer, rows, on_device, keepalive)"""
        if isinstance(support, (int, np.integer)):
            return C.c_void_p(int(support)), int(n_support_rows), 1, None
        s = np.ascontiguousarray(support, dtype=np.int32).reshape(-1, self.max_len)
        return C.c_void_p(s.ctypes.data), s.shape[0], 0, s

    def _adapt(self, support, n_support_rows, inner_steps, inner_lr, support_len):
        """the support arguments of a MAML decode / score call -> (masked, argument tuple, keepalive); support_len (host int32
        [rows], or a device address with a device support): the _masked entry point"""
        sp, rows, dev, keep = self._support(support, n_support_rows)
        if support_len is None:
            return False, (sp, rows, int(inner_steps), float(inner_lr), dev), keep
        sl, keep_len = self._len_ptr(support_len, rows, dev)
        return True, (sp, sl, rows, int(inner_steps), float(inner_lr), dev), (keep, keep_len)

    def _gen_args(self, n_seq, num, temperature, top_k, seed, primer):
        P, on_device, pp, keep = self._primer(primer, n_seq, ('n_seq', 'sequence'))
        return self.gen_config(n_seq, num, temperature, top_k, seed, P, on_device), pp, keep

    @staticmethod
    def gen_filters(top_p=0.0, min_p=0.0, repetition_penalty=1.0, repeat_window=0):
        """the fsmg_gen_filters struct, or None when every filter is off (include/fsmg.h: neutral filters)"""
        if top_p in (0.0, 1.0) and min_p == 0.0 and repetition_penalty in (0.0, 1.0):
            return None
        return FsmgGenFilters(version=FSMG_GEN_FILTERS_VERSION, top_p=float(top_p), min_p=float(min_p),
                              repetition_penalty=float(repetition_penalty), repeat_window=int(repeat_window))

    # -- constrained decoding (include/fsmg.h fsmg_constraint_*) -----------------------------------
    def new_constraint(self, con):
        """upload a data.constraints.Constraints -> DeviceConstraint"""
        return DeviceConstraint(self, con)

    def _constraint(self, con):
        """a DeviceConstraint of this model for `con` (a host Constraints is uploaded once and kept with the model)"""
        if isinstance(con, DeviceConstraint):
            if con._model is not self or not getattr(con, '_con', None):
                raise ValueError('constraints must be an open DeviceConstraint of this model')
            return con
        cache = self.__dict__.setdefault('_constraints', {})
        if id(con) not in cache:
            cache[id(con)] = (con, DeviceConstraint(self, con))       # (the host object is kept: its id stays its own)
        return cache[id(con)][1]

    def _constrained(self, call, head, tail, dc, n_seq, num, logprobs, cstate, return_cstate):
        """one of the three *_constrained entry points: call(g, f, con, cstate*, ...); -> tokens (, log-probs) (, cstate dict)"""
        rows = int(n_seq)
        cs = cstate or {}
        st = np.ascontiguousarray(cs['state'], dtype=np.int32).reshape(rows).copy() if cs.get('state') is not None else None
        op = (np.ascontiguousarray(cs['open'], dtype=np.uint32).reshape(rows, dc.n_words).copy()
              if cs.get('open') is not None else None)
        de = np.ascontiguousarray(cs['dead_ends'], dtype=np.int32).reshape(rows).copy() if cs.get('dead_ends') is not None else None
        io = None
        if cstate is not None or return_cstate:
            # the arrays are read at the start and written at the end; one that is not given holds the library's default for a NULL
            # input (start state, every slot closed, zero dead ends)
            if st is None or op is None or de is None:
                info_state = self._default_cstate(dc, rows)
                st = info_state['state'] if st is None else st
                op = info_state['open'] if op is None else op
                de = info_state['dead_ends'] if de is None else de
            io = FsmgConstraintState(state=st.ctypes.data, open=op.ctypes.data if op.size else None, dead_ends=de.ctypes.data)
        toks = np.empty((rows, int(num)), np.int32)
        lp = np.empty((rows, int(num)), np.float32) if logprobs else None
        call(*head, dc._con, C.byref(io) if io is not None else None, *tail, toks.ctypes.data_as(_I32P), _f32p(lp) if logprobs else None)
        out = (toks, lp) if logprobs else (toks,)
        if return_cstate:
            out = out + (dict(state=st, open=op, dead_ends=de),)
        return out if len(out) > 1 else out[0]

    @staticmethod
    def _default_cstate(dc, rows):
        return dict(state=np.full(rows, dc.start_state, np.int32), open=np.zeros((rows, dc.n_words), np.uint32),
                    dead_ends=np.zeros(rows, np.int32))

    def _generate(self, adapt, n_seq, num, temperature, top_k, seed, primer, logprobs, filters, masked=False):
        """fsmg_generate (adapt = ()) or fsmg_maml_generate (adapt = its support arguments), the _filtered entry point when a
        filter is on; masked: fsmg_maml_generate_filtered_masked (adapt holds the support lengths; a NULL filter struct: none)"""
        g, pp, _keep = self._gen_args(n_seq, num, temperature, top_k, seed, primer)
        f = self.gen_filters(*filters)
        toks = np.empty((int(n_seq), int(num)), np.int32)
        lp = np.empty((int(n_seq), int(num)), np.float32) if logprobs else None
        name = ('fsmg_maml_generate' if adapt else 'fsmg_generate') + ('' if f is None else '_filtered')
        head = (C.byref(g),) if f is None else (C.byref(g), C.byref(f))
        if masked:
            name, head = 'fsmg_maml_generate_filtered_masked', (C.byref(g), C.byref(f) if f is not None else None)
        self._ck(getattr(self._lib, name)(self._h, *head, *adapt, pp, toks.ctypes.data_as(_I32P), _f32p(lp) if logprobs else None))
        return (toks, lp) if logprobs else toks

    def generate(self, n_seq, num, temperature=1.0, top_k=0, seed=0, primer=None, logprobs=False, top_p=0.0, min_p=0.0,
                 repetition_penalty=1.0, repeat_window=0, state=None, constraints=None, cstate=None, return_cstate=False):
        """n_seq independent samples of num tokens -> int32 [n_seq, num] (, float32 [n_seq, num] log-probs with logprobs=True).
        primer: int32 [n_seq, P] (or [P] for every row) continued by each row, or (device address, P).  top_p, min_p,
        repetition_penalty, repeat_window: the sampling filters of fsmg_generate_filtered (all off: fsmg_generate).
        state: a DecodeState of n_seq rows to continue and leave advanced (fsmg_dstate_generate; no primer then: feed it).
        constraints: a data.constraints.Constraints or a DeviceConstraint (fsmg_generate_constrained /
        fsmg_dstate_generate_constrained); cstate: the rows' constraint states to start from, a dict with any of 'state' int32
        [n_seq], 'open' uint32 [n_seq, words], 'dead_ends' int32 [n_seq]; return_cstate: the states after the call, such a dict,
        as the last element of the result."""
        filters = (top_p, min_p, repetition_penalty, repeat_window)
        if constraints is None and (cstate is not None or return_cstate):
            raise ValueError('cstate / return_cstate need constraints')
        if state is not None and primer is not None:
            raise ValueError('a state takes no primer: feed it first')
        if state is not None and int(n_seq) != state.rows:
            raise ValueError('n_seq %d is not the row count of the state (%d)' % (int(n_seq), state.rows))
        if constraints is not None:
            dc = self._constraint(constraints)
            f = self.gen_filters(*filters)
            fp = C.byref(f) if f is not None else None
            if state is None:
                g, pp, _keep = self._gen_args(n_seq, num, temperature, top_k, seed, primer)
                return self._constrained(lambda *a: self._ck(self._lib.fsmg_generate_constrained(self._h, *a)), (C.byref(g), fp), (pp,),
                                         dc, n_seq, num, logprobs, cstate, return_cstate)
            g = self.gen_config(n_seq, num, temperature, top_k, seed)
            return self._constrained(lambda *a: state._call(self._lib.fsmg_dstate_generate_constrained, *a), (C.byref(g), fp), (), dc,
                                     n_seq, num, logprobs, cstate, return_cstate)
        if state is None:
            return self._generate((), n_seq, num, temperature, top_k, seed, primer, logprobs, filters)
        g = self.gen_config(n_seq, num, temperature, top_k, seed)
        f = self.gen_filters(*filters)
        toks = np.empty((int(n_seq), int(num)), np.int32)
        lp = np.empty((int(n_seq), int(num)), np.float32) if logprobs else None
        state._call(self._lib.fsmg_dstate_generate, C.byref(g), C.byref(f) if f is not None else None, toks.ctypes.data_as(_I32P),
                    _f32p(lp) if logprobs else None)
        return (toks, lp) if logprobs else toks

    # -- decode states (include/fsmg.h fsmg_dstate_*) ---------------------------------------------------------
    def new_state(self, rows, history=1024):
        """a fresh DecodeState of `rows` rows that keeps the last `history` context tokens (the repetition penalty's reach)"""
        return DecodeState(self, rows, history)

    def feed(self, state, tokens, logprobs=False):
        """read given tokens int32 [rows, n] (one [n] row: for every row; or (device address, n)) into the state; ids in
        [0, input_size], the start word included.  logprobs=True -> float32 [rows, n], the model log-probability of each token
        given everything the row has read; else None, and no logits are computed."""
        if isinstance(tokens, tuple):                 # (device address, n)
            tp, n, dev, _keep = C.c_void_p(int(tokens[0])), int(tokens[1]), 1, None
        else:
            a = np.ascontiguousarray(tokens, dtype=np.int32)
            if a.ndim == 1:
                a = np.ascontiguousarray(np.broadcast_to(a, (state.rows, a.size)))
            if a.ndim != 2 or a.shape[0] != state.rows:
                raise ValueError('tokens must be [%d, n] (or one [n] row for every row), got %r' % (state.rows, a.shape))
            tp, n, dev, _keep = C.c_void_p(a.ctypes.data), a.shape[1], 0, a
        lp = np.empty((state.rows, n), np.float32) if logprobs else None
        state._call(self._lib.fsmg_dstate_feed, tp, n, dev, _f32p(lp) if logprobs else None)
        return lp

    # -- batched passes from a carried state (include/fsmg.h fsmg_*_state) ---------------------------------
    def _state_args(self, state, tokens, lengths):
        """-> (config, token pointer, length pointer or None, keepalives): tokens int32 [rows, max_len] (or a device address), lengths
        host int32 [rows] in [0, max_len] or None = every position"""
        if not isinstance(state, DecodeState) or state._model is not self:
            raise ValueError('state must be a DecodeState of this model')
        tp, dev, keep = _tok_ptr(tokens)
        if keep is not None and keep.shape != (state.rows, self.max_len):
            raise ValueError('tokens must be [%d, %d], got %r' % (state.rows, self.max_len, keep.shape))
        ln = None
        if lengths is not None:
            ln = np.ascontiguousarray(lengths, dtype=np.int32).reshape(-1)
            if ln.size != state.rows:
                raise ValueError('%d lengths for %d rows' % (ln.size, state.rows))
        c = FsmgStateConfig(version=FSMG_STATE_CONFIG_VERSION, tokens_on_device=dev)
        return c, tp, (ln.ctypes.data_as(_I32P) if ln is not None else None), (keep, ln)

    def score_state(self, state, tokens, lengths=None, rank=False, entropy=False, argmax=False):
        """fsmg_score's outputs for one segment read from `state`, which is left advanced: dict of 'logprob' float32 [rows, max_len],
        'row_nll' [rows] (over the scored positions; NaN for a row of length 0) and, on request, 'rank', 'entropy', 'argmax';
        everything behind a row's length is 0"""
        c, tp, lp, _keep = self._state_args(state, tokens, lengths)
        n = (state.rows, self.max_len)
        out = dict(logprob=np.empty(n, np.float32), row_nll=np.empty(state.rows, np.float32))
        if rank:
            out['rank'] = np.empty(n, np.int32)
        if entropy:
            out['entropy'] = np.empty(n, np.float32)
        if argmax:
            out['argmax'] = np.empty(n, np.int32)
        state._call(self._lib.fsmg_score_state, C.byref(c), tp, lp, _f32p(out['logprob']),
                    out['rank'].ctypes.data_as(_I32P) if rank else None, _f32p(out['entropy']) if entropy else None,
                    out['argmax'].ctypes.data_as(_I32P) if argmax else None, _f32p(out['row_nll']))
        return out

    def eval_step_state(self, state, tokens, lengths=None):
        """-> (nll, n_valid): the segment's NLL over its n_valid scored positions; advances the state.  Segments of one stream combine
        as sum(nll_i * n_i) / sum(n_i)."""
        c, tp, lp, _keep = self._state_args(state, tokens, lengths)
        nll, nv = C.c_float(), C.c_int32()
        state._call(self._lib.fsmg_eval_step_state, C.byref(c), tp, lp, C.byref(nll), C.byref(nv))
        return nll.value, int(nv.value)

    def forward_backward_state(self, state, tokens, lengths=None):
        """loss and gradients of the segment with the incoming state held constant (truncated BPTT); apply_update follows, as after
        forward_backward_masked.  Advances the state."""
        c, tp, lp, _keep = self._state_args(state, tokens, lengths)
        state._call(self._lib.fsmg_forward_backward_state, C.byref(c), tp, lp)

    def train_step_state(self, state, tokens, lengths=None):
        """the fused step on one segment -> its loss; advances the state"""
        c, tp, lp, _keep = self._state_args(state, tokens, lengths)
        loss = C.c_float()
        state._call(self._lib.fsmg_train_step_state, C.byref(c), tp, lp, C.byref(loss))
        return loss.value

    def maml_generate(self, support, num, inner_steps, inner_lr, n_seq=1, temperature=1.0, top_k=0, seed=0, primer=None,
                      logprobs=False, n_support_rows=None, top_p=0.0, min_p=0.0, repetition_penalty=1.0, repeat_window=0,
                      support_len=None, constraints=None, cstate=None, return_cstate=False):
        """adapt on support [rows, max_len] (numpy, or a device address with n_support_rows), generate at theta', restore theta.
        support_len int32 [rows]: adapt over the positions inside each support song only (fsmg_maml_generate_filtered_masked).
        constraints, cstate, return_cstate: as in generate (fsmg_maml_generate_constrained)"""
        masked, adapt, _keep = self._adapt(support, n_support_rows, inner_steps, inner_lr, support_len)
        if constraints is None and (cstate is not None or return_cstate):
            raise ValueError('cstate / return_cstate need constraints')
        if constraints is not None:
            dc = self._constraint(constraints)
            f = self.gen_filters(top_p, min_p, repetition_penalty, repeat_window)
            g, pp, _keep_p = self._gen_args(n_seq, num, temperature, top_k, seed, primer)
            sup = adapt if masked else (adapt[0], None) + adapt[1:]       # (support, support_len or NULL, rows, steps, lr, on device)
            return self._constrained(lambda *a: self._ck(self._lib.fsmg_maml_generate_constrained(self._h, *a)),
                                     (C.byref(g), C.byref(f) if f is not None else None), sup + (pp,), dc, n_seq, num, logprobs, cstate,
                                     return_cstate)
        if not masked:
            return self._generate(adapt, n_seq, num, temperature, top_k, seed, primer, logprobs,
                                  (top_p, min_p, repetition_penalty, repeat_window))
        return self._generate(adapt, n_seq, num, temperature, top_k, seed, primer, logprobs,
                              (top_p, min_p, repetition_penalty, repeat_window), masked=True)

    # -- batched on-device beam search (include/fsmg.h fsmg_beam_search) ----------------------------------------
    @staticmethod
    def beam_config(n_groups, beam_width, num, primer_len=0, primer_on_device=0):
        return FsmgBeamConfig(version=FSMG_BEAM_CONFIG_VERSION, n_groups=int(n_groups), beam_width=int(beam_width), num=int(num),
                              primer_len=int(primer_len), primer_on_device=int(primer_on_device))

    def _beam_search(self, adapt, num, beam_width, n_groups, primer, logprobs, masked=False):
        """fsmg_beam_search (adapt = ()) or fsmg_maml_beam_search (adapt = its support arguments; masked: with their lengths)"""
        P, on_device, pp, _keep = self._primer(primer, n_groups, ('n_groups', 'group'))
        b = self.beam_config(n_groups, beam_width, num, P, on_device)
        G, W, num = int(n_groups), int(beam_width), int(num)
        toks = np.empty((G, W, num), np.int32)
        scores = np.empty((G, W), np.float32)
        lp = np.empty((G, W, num), np.float32) if logprobs else None
        fn = self._lib.fsmg_maml_beam_search if adapt else self._lib.fsmg_beam_search
        if masked:
            fn = self._lib.fsmg_maml_beam_search_masked
        self._ck(fn(self._h, C.byref(b), *adapt, pp, toks.ctypes.data_as(_I32P), _f32p(scores), _f32p(lp) if logprobs else None))
        return (toks, scores, lp) if logprobs else (toks, scores)

    def _beam_constrained(self, call, head, tail, dc, n_groups, beam_width, num, logprobs, cstate, return_cstate):
        """one of the three *_beam_search_constrained entry points: call(*head, con, cstate_in*, cstate_out*, *tail, tokens, scores,
        log-probs); cstate is per group, the returned dict per hypothesis ([G, W, ...])"""
        G, W, num = int(n_groups), int(beam_width), int(num)
        cs = cstate or {}
        keep = []

        def arr(key, dtype, shape):
            if cs.get(key) is None:
                return None
            a = np.ascontiguousarray(cs[key], dtype=dtype).reshape(shape)
            keep.append(a)
            return a.ctypes.data if a.size else None
        cin = None
        if cstate is not None:
            cin = FsmgConstraintState(state=arr('state', np.int32, (G,)), open=arr('open', np.uint32, (G, dc.n_words)),
                                      dead_ends=arr('dead_ends', np.int32, (G,)))
        out_cs = cout = None
        if return_cstate:
            out_cs = dict(state=np.empty((G, W), np.int32), open=np.empty((G, W, dc.n_words), np.uint32),
                          dead_ends=np.empty((G, W), np.int32))
            cout = FsmgConstraintState(state=out_cs['state'].ctypes.data, open=out_cs['open'].ctypes.data if dc.n_words else None,
                                       dead_ends=out_cs['dead_ends'].ctypes.data)
        toks = np.empty((G, W, num), np.int32)
        scores = np.empty((G, W), np.float32)
        lp = np.empty((G, W, num), np.float32) if logprobs else None
        call(*head, dc._con, C.byref(cin) if cin is not None else None, C.byref(cout) if cout is not None else None, *tail,
             toks.ctypes.data_as(_I32P), _f32p(scores), _f32p(lp) if logprobs else None)
        out = (toks, scores, lp) if logprobs else (toks, scores)
        return out + (out_cs,) if return_cstate else out

    def beam_search(self, num, beam_width, n_groups=1, primer=None, logprobs=False, state=None, constraints=None, cstate=None,
                    return_cstate=False):
        """n_groups independent beam searches of width beam_width, num tokens each -> tokens int32 [G, W, num], scores float32
        [G, W] (, log-probs float32 [G, W, num] with logprobs=True), each group's hypotheses best first.  primer: int32 [G, P]
        (or [P] for every group) continued by every hypothesis of its group, or (device address, P).
        state: a DecodeState of n_groups rows, group g searching on from its row g (fsmg_dstate_beam_search; the state is only read).
        constraints: a data.constraints.Constraints or a DeviceConstraint (fsmg_beam_search_constrained /
        fsmg_dstate_beam_search_constrained); cstate: the groups' constraint states to start from, a dict with any of 'state' int32
        [G], 'open' uint32 [G, words], 'dead_ends' int32 [G]; return_cstate: the hypotheses' final states, a dict of 'state' [G, W],
        'open' [G, W, words], 'dead_ends' [G, W], as the last element of the result."""
        if constraints is None and (cstate is not None or return_cstate):
            raise ValueError('cstate / return_cstate need constraints')
        if state is not None and primer is not None:
            raise ValueError('a state takes no primer: feed it first')
        if state is not None and int(n_groups) != state.rows:
            raise ValueError('n_groups %d is not the row count of the state (%d)' % (int(n_groups), state.rows))
        if constraints is not None:
            dc = self._constraint(constraints)
            if state is None:
                P, on_device, pp, _keep = self._primer(primer, n_groups, ('n_groups', 'group'))
                b = self.beam_config(n_groups, beam_width, num, P, on_device)
                return self._beam_constrained(lambda *a: self._ck(self._lib.fsmg_beam_search_constrained(self._h, *a)), (C.byref(b),),
                                              (pp,), dc, n_groups, beam_width, num, logprobs, cstate, return_cstate)
            b = self.beam_config(n_groups, beam_width, num)
            return self._beam_constrained(lambda *a: state._call(self._lib.fsmg_dstate_beam_search_constrained, *a), (C.byref(b),), (),
                                          dc, n_groups, beam_width, num, logprobs, cstate, return_cstate)
        if state is None:
            return self._beam_search((), num, beam_width, n_groups, primer, logprobs)
        if primer is not None:
            raise ValueError('a state takes no primer: feed it first')
        if int(n_groups) != state.rows:
            raise ValueError('n_groups %d is not the row count of the state (%d)' % (int(n_groups), state.rows))
        b = self.beam_config(n_groups, beam_width, num)
        G, W, num = int(n_groups), int(beam_width), int(num)
        toks = np.empty((G, W, num), np.int32)
        scores = np.empty((G, W), np.float32)
        lp = np.empty((G, W, num), np.float32) if logprobs else None
        state._call(self._lib.fsmg_dstate_beam_search, C.byref(b), toks.ctypes.data_as(_I32P), _f32p(scores),
                    _f32p(lp) if logprobs else None)
        return (toks, scores, lp) if logprobs else (toks, scores)

    def maml_beam_search(self, support, num, inner_steps, inner_lr, beam_width, n_groups=1, primer=None, logprobs=False,
                         n_support_rows=None, support_len=None, constraints=None, cstate=None, return_cstate=False):
        """adapt on support [rows, max_len] (numpy, or a device address with n_support_rows), beam search at theta', restore theta.
        support_len int32 [rows]: adapt over the positions inside each support song only (fsmg_maml_beam_search_masked).
        constraints, cstate, return_cstate: as in beam_search (fsmg_maml_beam_search_constrained)"""
        masked, adapt, _keep = self._adapt(support, n_support_rows, inner_steps, inner_lr, support_len)
        if constraints is None and (cstate is not None or return_cstate):
            raise ValueError('cstate / return_cstate need constraints')
        if constraints is not None:
            dc = self._constraint(constraints)
            P, on_device, pp, _keep_p = self._primer(primer, n_groups, ('n_groups', 'group'))
            b = self.beam_config(n_groups, beam_width, num, P, on_device)
            sup = adapt if masked else (adapt[0], None) + adapt[1:]       # (support, support_len or NULL, rows, steps, lr, on device)
            return self._beam_constrained(lambda *a: self._ck(self._lib.fsmg_maml_beam_search_constrained(self._h, *a)), (C.byref(b),),
                                          sup + (pp,), dc, n_groups, beam_width, num, logprobs, cstate, return_cstate)
        if not masked:
            return self._beam_search(adapt, num, beam_width, n_groups, primer, logprobs)
        return self._beam_search(adapt, num, beam_width, n_groups, primer, logprobs, masked=True)

    # -- scoring of given songs (include/fsmg.h fsmg_score) -----------------------------------------------------
    @staticmethod
    def score_config(n_rows, nll_first=0, nll_count=0, pass_rows=0, tokens_on_device=0):
        return FsmgScoreConfig(version=FSMG_SCORE_CONFIG_VERSION, n_rows=int(n_rows), tokens_on_device=int(tokens_on_device),
                               nll_first=int(nll_first), nll_count=int(nll_count), pass_rows=int(pass_rows))

    def _lengths(self, lengths, n, what='lengths'):
        """the true lengths of n rows as int32 [n], each in [1, max_len]; ValueError otherwise (before the library is called)"""
        a = np.ascontiguousarray(lengths, dtype=np.int32).reshape(-1)
        if a.size != n:
            raise ValueError('%s must hold %d values, got %r' % (what, n, np.shape(lengths)))
        if a.size and (a.min() < 1 or a.max() > self.max_len):
            raise ValueError('every value of %s must be in [1, %d]' % (what, self.max_len))
        return a

    def _score(self, adapt, tokens, n_rows, logprob, rank, entropy, argmax, row_nll, nll_first, nll_count, pass_rows, lengths=None,
               masked=False):
        """fsmg_score (adapt = ()), fsmg_maml_score (adapt = its support arguments), fsmg_score_masked (lengths) or
        fsmg_maml_score_masked (masked: adapt holds the support lengths; lengths: the scored songs' own, or None)"""
        if isinstance(tokens, (int, np.integer)):
            tp, dev, _keep, R = C.c_void_p(int(tokens)), 1, None, int(n_rows)
        else:
            a = np.ascontiguousarray(tokens, dtype=np.int32)
            if a.ndim == 0 or a.shape[-1] != self.max_len:
                raise ValueError('tokens %r do not match max_len=%d' % (a.shape, self.max_len))
            a = a.reshape(-1, self.max_len)
            tp, dev, _keep, R = C.c_void_p(a.ctypes.data), 0, a, a.shape[0]
        c = self.score_config(R, nll_first, nll_count, pass_rows, dev)
        T = self.max_len
        out = {}
        if logprob:
            out['logprob'] = np.empty((R, T), np.float32)
        if rank:
            out['rank'] = np.empty((R, T), np.int32)
        if entropy:
            out['entropy'] = np.empty((R, T), np.float32)
        if argmax:
            out['argmax'] = np.empty((R, T), np.int32)
        if row_nll:
            out['row_nll'] = np.empty(R, np.float32)
        f = lambda k: _f32p(out[k]) if k in out else None
        i = lambda k: out[k].ctypes.data_as(_I32P) if k in out else None
        if masked:
            ln = self._lengths(lengths, R) if lengths is not None else None
            self._ck(self._lib.fsmg_maml_score_masked(self._h, C.byref(c), *adapt, tp, ln.ctypes.data_as(_I32P) if ln is not None else None,
                                                      f('logprob'), i('rank'), f('entropy'), i('argmax'), f('row_nll')))
            return out
        if lengths is not None:
            ln = self._lengths(lengths, R)
            self._ck(self._lib.fsmg_score_masked(self._h, C.byref(c), tp, ln.ctypes.data_as(_I32P), f('logprob'), i('rank'), f('entropy'),
                                                 i('argmax'), f('row_nll')))
            return out
        fn = self._lib.fsmg_maml_score if adapt else self._lib.fsmg_score
        self._ck(fn(self._h, C.byref(c), *adapt, tp, f('logprob'), i('rank'), f('entropy'), i('argmax'), f('row_nll')))
        return out

    def score(self, tokens, logprob=True, rank=False, entropy=False, argmax=False, row_nll=True, nll_first=0, nll_count=0,
              pass_rows=0, n_rows=None, lengths=None):
        """Per-token statistics of given songs: tokens int32 [R, max_len] (or a device address with n_rows) -> a dict with the
        requested arrays: 'logprob' float32 [R, T] (model log-probability of each token), 'rank' int32 [R, T] (0-based rank of the
        true token, lower index first on ties), 'entropy' float32 [R, T] (predictive entropy), 'argmax' int32 [R, T], 'row_nll'
        float32 [R] (mean NLL of positions nll_first .. nll_first + nll_count - 1; nll_count 0 = to the end).  pass_rows: rows
        per device pass (0 = 128).  lengths int32 [R], each in [1, max_len]: position t of row r is scored iff t < lengths[r]; every
        per-token array is 0 behind a song's end and row_nll averages over the scored positions of its window (NaN if none)."""
        return self._score((), tokens, n_rows, logprob, rank, entropy, argmax, row_nll, nll_first, nll_count, pass_rows, lengths)

    def maml_score(self, support, tokens, inner_steps, inner_lr, logprob=True, rank=False, entropy=False, argmax=False, row_nll=True,
                   nll_first=0, nll_count=0, pass_rows=0, n_rows=None, n_support_rows=None, support_len=None, lengths=None):
        """adapt on support [rows, max_len] (numpy, or a device address with n_support_rows), score at theta', restore theta.
        support_len int32 [rows]: adapt over the positions inside each support song only; lengths int32 [R]: the scored songs' own,
        as in score() -- either one selects fsmg_maml_score_masked"""
        if support_len is None and lengths is not None:
            raise ValueError('maml_score(lengths=) goes with support_len= (the masked adaptation)')
        masked, adapt, _keep = self._adapt(support, n_support_rows, inner_steps, inner_lr, support_len)
        if not masked:
            return self._score(adapt, tokens, n_rows, logprob, rank, entropy, argmax, row_nll, nll_first, nll_count, pass_rows)
        return self._score(adapt, tokens, n_rows, logprob, rank, entropy, argmax, row_nll, nll_first, nll_count, pass_rows, lengths,
                           masked=True)

    # -- support-set neural cache (include/fsmg.h fsmg_cache_*) ---------------------------------------------------
    @staticmethod
    def cache_score_config(n_rows, thetas, lambdas, nll_first=0, nll_count=0, pass_rows=0, tokens_on_device=0):
        """FsmgCacheScoreConfig for thetas (1..8 finite values >= 0) and lambdas (1..16 values in [0, 1]); ValueError otherwise"""
        th = np.atleast_1d(np.asarray(thetas, np.float32))
        la = np.atleast_1d(np.asarray(lambdas, np.float32))
        if th.ndim != 1 or not 1 <= th.size <= FSMG_CACHE_MAX_THETA or not np.all(np.isfinite(th)) or np.any(th < 0):
            raise ValueError('thetas must be 1..%d finite values >= 0, got %r' % (FSMG_CACHE_MAX_THETA, thetas))
        if la.ndim != 1 or not 1 <= la.size <= FSMG_CACHE_MAX_LAMBDA or not np.all((la >= 0) & (la <= 1)):
            raise ValueError('lambdas must be 1..%d values in [0, 1], got %r' % (FSMG_CACHE_MAX_LAMBDA, lambdas))
        c = FsmgCacheScoreConfig(version=FSMG_CACHE_SCORE_CONFIG_VERSION, n_rows=int(n_rows), tokens_on_device=int(tokens_on_device),
                                 nll_first=int(nll_first), nll_count=int(nll_count), pass_rows=int(pass_rows), n_theta=th.size,
                                 n_lambda=la.size)
        c.thetas[:th.size] = th.tolist()
        c.lambdas[:la.size] = la.tolist()
        return c

    def _rows(self, tokens, n_rows):
        """host [.., max_len] tokens or a device address with n_rows -> (void*, on_device, keepalive, rows)"""
        if isinstance(tokens, (int, np.integer)):
            return C.c_void_p(int(tokens)), 1, None, int(n_rows)
        a = np.ascontiguousarray(tokens, dtype=np.int32)
        if a.ndim == 0 or a.shape[-1] != self.max_len:
            raise ValueError('tokens %r do not match max_len=%d' % (a.shape, self.max_len))
        a = a.reshape(-1, self.max_len)
        return C.c_void_p(a.ctypes.data), 0, a, a.shape[0]

    def cache_build(self, tokens, n_groups=1, pass_rows=0, n_rows=None, lengths=None):
        """Read support songs int32 [rows, max_len] ([groups, K, max_len] works too; or a device address with n_rows) into a new
        FsmgCache of n_groups groups: row r belongs to group r // (rows // n_groups), and entry (r % rows_per_group) * T + t holds
        the top-layer hidden state that predicts token t of the row, with that token as its value.  lengths int32 [rows], each in
        [1, max_len]: only positions t < lengths[r] are filed, a group's entries packed without gaps (a ragged cache: counts())."""
        tp, dev, _keep, R = self._rows(tokens, n_rows)
        c = FsmgCacheConfig(version=FSMG_CACHE_CONFIG_VERSION, n_rows=R, n_groups=int(n_groups), tokens_on_device=dev,
                            pass_rows=int(pass_rows))
        out = _P()
        if lengths is not None:
            ln = self._lengths(lengths, R)
            self._ck(self._lib.fsmg_cache_build_masked(self._h, C.byref(c), tp, ln.ctypes.data_as(_I32P), C.byref(out)))
            return FsmgCache(self, out)
        self._ck(self._lib.fsmg_cache_build(self._h, C.byref(c), tp, C.byref(out)))
        return FsmgCache(self, out)

    def cache_from(self, keys, values, counts=None):
        """a new FsmgCache from host arrays: keys float32 [groups, entries, H], values int32 [groups, entries]; counts int32
        [groups], each in [1, entries]: group g holds its first counts[g] entries and what lies behind them is not read"""
        k = np.ascontiguousarray(keys, dtype=np.float32)
        v = np.ascontiguousarray(values, dtype=np.int32)
        if k.ndim != 3 or k.shape[2] != int(self.cfg.hidden_size) or v.shape != k.shape[:2]:
            raise ValueError('keys must be [groups, entries, %d] and values [groups, entries], got %r and %r'
                             % (int(self.cfg.hidden_size), k.shape, v.shape))
        out = _P()
        if counts is not None:
            n = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
            if n.size != k.shape[0] or n.min() < 1 or n.max() > k.shape[1]:
                raise ValueError('counts must hold %d values in [1, %d], got %r' % (k.shape[0], k.shape[1], counts))
            self._ck(self._lib.fsmg_cache_create_from_counts(self._h, k.shape[0], k.shape[1], n.ctypes.data_as(_I32P), _f32p(k),
                                                             v.ctypes.data_as(_I32P), C.byref(out)))
            return FsmgCache(self, out)
        self._ck(self._lib.fsmg_cache_create_from(self._h, k.shape[0], k.shape[1], _f32p(k), v.ctypes.data_as(_I32P), C.byref(out)))
        return FsmgCache(self, out)

    def cache_attend(self, cache, queries, targets, thetas, group=None):
        """p_cache of raw query vectors: queries float32 [n, H], targets int32 [n], group int32 [n] (None: all in group 0), thetas
        1..8 values >= 0 -> float32 [n_theta, n]: the softmax(theta q . k) mass of the entries of the query's group that hold its
        target, exactly 0 when none does."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        y = np.ascontiguousarray(targets, dtype=np.int32)
        th = np.atleast_1d(np.ascontiguousarray(thetas, dtype=np.float32))
        if q.ndim != 2 or q.shape[1] != int(self.cfg.hidden_size) or y.shape != (q.shape[0],):
            raise ValueError('queries must be [n, %d] and targets [n], got %r and %r' % (int(self.cfg.hidden_size), q.shape, y.shape))
        g = None
        if group is not None:
            g = np.ascontiguousarray(group, dtype=np.int32)
            if g.shape != y.shape:
                raise ValueError('group must be [%d], got %r' % (y.size, g.shape))
        out = np.empty((th.size, q.shape[0]), np.float32)
        self._ck(self._lib.fsmg_cache_attend(self._h, cache._ptr(), q.shape[0], _f32p(q), y.ctypes.data_as(_I32P),
                    g.ctypes.data_as(_I32P) if g is not None else None, _f32p(th), th.size, _f32p(out)))
        return out

    def cache_score(self, cache, tokens, thetas, lambdas, group=None, logprob=True, cache_prob=False, lstm_logprob=False, row_nll=True,
                    nll_first=0, nll_count=0, pass_rows=0, n_rows=None, lengths=None):
        """score() with a cache beside the model: tokens int32 [R, max_len] (or a device address with n_rows), row r attending
        over group group[r] of the cache (None: group 0) -> a dict with the requested arrays: 'logprob' float32 [n_theta, n_lambda, R,
        T] (log of the (1 - lambda, lambda) mixture of the model's and the cache's probability of each token), 'cache_prob' float32
        [n_theta, R, T], 'lstm_logprob' float32 [R, T] (score()'s 'logprob'), 'row_nll' float32 [n_theta, n_lambda, R].  The whole
        (theta, lambda) grid costs one device pass.  lengths int32 [R]: as score(); a query behind its song's end costs no attention."""
        tp, dev, _keep, R = self._rows(tokens, n_rows)
        c = self.cache_score_config(R, thetas, lambdas, nll_first, nll_count, pass_rows, dev)
        g = None
        if group is not None:
            g = np.ascontiguousarray(group, dtype=np.int32)
            if g.shape != (R,):
                raise ValueError('group must be [%d], got %r' % (R, g.shape))
        T, NT, NL = self.max_len, c.n_theta, c.n_lambda
        out = {}
        if logprob:
            out['logprob'] = np.empty((NT, NL, R, T), np.float32)
        if cache_prob:
            out['cache_prob'] = np.empty((NT, R, T), np.float32)
        if lstm_logprob:
            out['lstm_logprob'] = np.empty((R, T), np.float32)
        if row_nll:
            out['row_nll'] = np.empty((NT, NL, R), np.float32)
        f = lambda k: _f32p(out[k]) if k in out else None
        if lengths is not None:
            ln = self._lengths(lengths, R)
            self._ck(self._lib.fsmg_cache_score_masked(self._h, cache._ptr(), C.byref(c), tp, ln.ctypes.data_as(_I32P),
                                                       g.ctypes.data_as(_I32P) if g is not None else None, f('logprob'), f('cache_prob'),
                                                       f('lstm_logprob'), f('row_nll')))
            return out
        self._ck(self._lib.fsmg_cache_score(self._h, cache._ptr(), C.byref(c), tp, g.ctypes.data_as(_I32P) if g is not None else None,
                                            f('logprob'), f('cache_prob'), f('lstm_logprob'), f('row_nll')))
        return out

    def cache_eval_step(self, support, query, theta, lam, support_len=None, query_len=None):
        """support int32 [N, K, max_len], query int32 [N, Q, max_len] -> the mean NLL of the query tokens under the mixture, artist
        a's query songs attending over a cache built from artist a's support songs (eval_step with the support set used)"""
        s = np.ascontiguousarray(support, dtype=np.int32)
        q = np.ascontiguousarray(query, dtype=np.int32)
        if s.ndim != 3 or q.ndim != 3 or s.shape[0] != q.shape[0] or s.shape[2] != self.max_len or q.shape[2] != self.max_len:
            raise ValueError('support %r / query %r must be [N, K, %d] and [N, Q, %d]' % (s.shape, q.shape, self.max_len, self.max_len))
        nll = C.c_float()
        if (support_len is None) != (query_len is None):
            raise ValueError('support_len and query_len go together')
        if support_len is not None:     # the padding-masked form: ragged groups, the mean over the scored positions
            sl = self._lengths(support_len, s.shape[0] * s.shape[1], 'support_len')
            ql = self._lengths(query_len, q.shape[0] * q.shape[1], 'query_len')
            self._ck(self._lib.fsmg_cache_eval_step_masked(self._h, C.c_void_p(s.ctypes.data), C.c_void_p(q.ctypes.data),
                                                           sl.ctypes.data_as(_I32P), ql.ctypes.data_as(_I32P), s.shape[0], s.shape[1],
                                                           q.shape[1], float(theta), float(lam), C.byref(nll)))
            return nll.value
        self._ck(self._lib.fsmg_cache_eval_step(self._h, C.c_void_p(s.ctypes.data), C.c_void_p(q.ctypes.data), s.shape[0], s.shape[1],
                                                q.shape[1], float(theta), float(lam), C.byref(nll)))
        return nll.value

    # -- cache-conditioned generation (include/fsmg.h fsmg_cache_generate) ----------------------------------------
    @staticmethod
    def cache_gen_config(theta, lam):
        return FsmgCacheGenConfig(version=FSMG_CACHE_GEN_CONFIG_VERSION, theta=float(theta), lambda_=float(lam))

    @staticmethod
    def _group(group, n):
        if group is None:
            return None
        g = np.ascontiguousarray(group, dtype=np.int32)
        if g.shape != (int(n),):
            raise ValueError('group must be [%d], got %r' % (int(n), g.shape))
        return g

    def cache_generate(self, cache, n_seq, num, theta, lam, group=None, state=None, temperature=1.0, top_k=0, seed=0, primer=None,
                       logprobs=False, top_p=0.0, min_p=0.0, repetition_penalty=1.0, repeat_window=0):
        """generate() drawing every token from the mixture (1 - lam) p_lstm + lam p_cache, row r attending over group group[r] of
        the cache (int32 [n_seq]; None: group 0) with sharpness theta.  lam = 0 is generate() bitwise.  state: a DecodeState of
        n_seq rows to continue and leave advanced (fsmg_dstate_cache_generate; no primer then).  The other keywords and the result
        are generate()'s; the log-probs are those of the mixture."""
        n_seq, num = int(n_seq), int(num)
        cc = self.cache_gen_config(theta, lam)
        g = self._group(group, n_seq)
        gp = g.ctypes.data_as(_I32P) if g is not None else None
        f = self.gen_filters(top_p, min_p, repetition_penalty, repeat_window)
        fp = C.byref(f) if f is not None else None
        toks = np.empty((n_seq, num), np.int32)
        lp = np.empty((n_seq, num), np.float32) if logprobs else None
        outs = (toks.ctypes.data_as(_I32P), _f32p(lp) if logprobs else None)
        if state is None:
            gc, pp, _keep = self._gen_args(n_seq, num, temperature, top_k, seed, primer)
            self._ck(self._lib.fsmg_cache_generate(self._h, cache._ptr(), C.byref(cc), C.byref(gc), fp, gp, pp, *outs))
        else:
            if primer is not None:
                raise ValueError('a state takes no primer: feed it first')
            if n_seq != state.rows:
                raise ValueError('n_seq %d is not the row count of the state (%d)' % (n_seq, state.rows))
            gc = self.gen_config(n_seq, num, temperature, top_k, seed)
            state._call(self._lib.fsmg_dstate_cache_generate, cache._ptr(), C.byref(cc), C.byref(gc), fp, gp, *outs)
        return (toks, lp) if logprobs else toks

    def cache_distribution(self, cache, queries, logits, theta, lam, group=None):
        """the mixture of given vectors: queries float32 [n, H], logits float32 [n, input_size + 1], group int32 [n] (None: all in
        group 0) -> a dict of 'cache_prob' float32 [n, V1] (p_cache of every column, exactly 0 where no entry holds it), 'logprob'
        float32 [n, V1] (the mixed log-probabilities a pick would read) and 'lse' float32 [n] (the logsumexp of each logits row)"""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        z = np.ascontiguousarray(logits, dtype=np.float32)
        H, V1 = int(self.cfg.hidden_size), int(self.cfg.input_size) + 1
        if q.ndim != 2 or q.shape[1] != H or z.shape != (q.shape[0], V1):
            raise ValueError('queries must be [n, %d] and logits [n, %d], got %r and %r' % (H, V1, q.shape, z.shape))
        n = q.shape[0]
        g = self._group(group, n)
        cc = self.cache_gen_config(theta, lam)
        out = dict(cache_prob=np.empty((n, V1), np.float32), logprob=np.empty((n, V1), np.float32), lse=np.empty(n, np.float32))
        self._ck(self._lib.fsmg_cache_distribution(self._h, cache._ptr(), C.byref(cc), n, _f32p(q), _f32p(z),
                                                   g.ctypes.data_as(_I32P) if g is not None else None, _f32p(out['cache_prob']),
                                                   _f32p(out['logprob']), _f32p(out['lse'])))
        return out

    # -- self-cache (include/fsmg.h fsmg_cache_self_*) -------------------------------------------------------------
    @staticmethod
    def cache_self_config(window):
        return FsmgCacheSelfConfig(version=FSMG_CACHE_SELF_CONFIG_VERSION, window=int(window))

    def cache_self_attend(self, vectors, values, thetas, window, cache=None, group=None):
        """p_cache of given rows under the self-cache: vectors float32 [n_rows, n_pos, H], values int32 [n_rows, n_pos] -- values[r,
        t] is the target of position t and the value of the row's own entry t.  Position t attends over its row's own entries
        max(0, t - window) .. t - 1 and, with a cache, over group group[r] of it (None: group 0), in one softmax -> float32
        [n_theta, n_rows, n_pos]; exactly 0 where no visible entry holds the target, position 0 without a cache included."""
        v = np.ascontiguousarray(vectors, dtype=np.float32)
        y = np.ascontiguousarray(values, dtype=np.int32)
        th = np.atleast_1d(np.ascontiguousarray(thetas, dtype=np.float32))
        if v.ndim != 3 or v.shape[2] != int(self.cfg.hidden_size) or y.shape != v.shape[:2]:
            raise ValueError('vectors must be [n_rows, n_pos, %d] and values [n_rows, n_pos], got %r and %r'
                             % (int(self.cfg.hidden_size), v.shape, y.shape))
        g = self._group(group, v.shape[0])
        sc = self.cache_self_config(window)
        out = np.empty((th.size,) + y.shape, np.float32)
        self._ck(self._lib.fsmg_cache_self_attend(self._h, cache._ptr() if cache is not None else None, C.byref(sc), v.shape[0], v.shape[1],
                                                  _f32p(v), y.ctypes.data_as(_I32P), g.ctypes.data_as(_I32P) if g is not None else None,
                                                  _f32p(th), th.size, _f32p(out)))
        return out

    def cache_self_score(self, tokens, thetas, lambdas, window, cache=None, group=None, logprob=True, cache_prob=False,
                         lstm_logprob=False, row_nll=True, nll_first=0, nll_count=0, pass_rows=0, n_rows=None, lengths=None):
        """cache_score() with every song's own history in the set: position t also attends over the hidden states of its own
        positions max(0, t - window) .. t - 1, each with the token that followed.  cache=None: the own history alone (group is then
        ignored; position 0 is scored by the model alone).  The keywords and the result are cache_score's."""
        tp, dev, _keep, R = self._rows(tokens, n_rows)
        c = self.cache_score_config(R, thetas, lambdas, nll_first, nll_count, pass_rows, dev)
        sc = self.cache_self_config(window)
        g = self._group(group, R)
        T, NT, NL = self.max_len, c.n_theta, c.n_lambda
        out = {}
        if logprob:
            out['logprob'] = np.empty((NT, NL, R, T), np.float32)
        if cache_prob:
            out['cache_prob'] = np.empty((NT, R, T), np.float32)
        if lstm_logprob:
            out['lstm_logprob'] = np.empty((R, T), np.float32)
        if row_nll:
            out['row_nll'] = np.empty((NT, NL, R), np.float32)
        f = lambda k: _f32p(out[k]) if k in out else None
        if lengths is not None:
            ln = self._lengths(lengths, R)
            self._ck(self._lib.fsmg_cache_self_score_masked(self._h, cache._ptr() if cache is not None else None, C.byref(c), C.byref(sc),
                                                            tp, ln.ctypes.data_as(_I32P), g.ctypes.data_as(_I32P) if g is not None else None,
                                                            f('logprob'), f('cache_prob'), f('lstm_logprob'), f('row_nll')))
            return out
        self._ck(self._lib.fsmg_cache_self_score(self._h, cache._ptr() if cache is not None else None, C.byref(c), C.byref(sc), tp,
                                                 g.ctypes.data_as(_I32P) if g is not None else None, f('logprob'), f('cache_prob'),
                                                 f('lstm_logprob'), f('row_nll')))
        return out

    def cache_self_generate(self, n_seq, num, theta, lam, window, cache=None, group=None, temperature=1.0, top_k=0, seed=0, primer=None,
                            logprobs=False, top_p=0.0, min_p=0.0, repetition_penalty=1.0, repeat_window=0):
        """cache_generate() with every row's own history in the set: at a generated position p the row also attends over the hidden
        states of its own positions max(0, p - window) .. p - 1 (primer positions included), each with the token that followed.
        cache=None: the own history alone (group is then ignored).  lam = 0 is generate() bitwise.  No decode-state variant."""
        n_seq, num = int(n_seq), int(num)
        cc, sc = self.cache_gen_config(theta, lam), self.cache_self_config(window)
        g = self._group(group, n_seq)
        gp = g.ctypes.data_as(_I32P) if g is not None else None
        f = self.gen_filters(top_p, min_p, repetition_penalty, repeat_window)
        fp = C.byref(f) if f is not None else None
        toks = np.empty((n_seq, num), np.int32)
        lp = np.empty((n_seq, num), np.float32) if logprobs else None
        gc, pp, _keep = self._gen_args(n_seq, num, temperature, top_k, seed, primer)
        self._ck(self._lib.fsmg_cache_self_generate(self._h, cache._ptr() if cache is not None else None, C.byref(cc), C.byref(sc),
                                                    C.byref(gc), fp, gp, pp, toks.ctypes.data_as(_I32P), _f32p(lp) if logprobs else None))
        return (toks, lp) if logprobs else toks

    def cache_self_distribution(self, queries, logits, self_keys, self_values, self_len, theta, lam, window, cache=None, group=None):
        """cache_distribution() over the union: row i also sees the last min(self_len[i], window) of its self_len[i] own entries
        (self_keys float32 [n, S, H], self_values int32 [n, S], self_len int32 [n], each in [0, S]).  An empty union (no cache,
        self_len 0) gives cache_prob 0 and logprob = the model's log-probabilities whatever lam is."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        z = np.ascontiguousarray(logits, dtype=np.float32)
        k = np.ascontiguousarray(self_keys, dtype=np.float32)
        v = np.ascontiguousarray(self_values, dtype=np.int32)
        ln = np.ascontiguousarray(self_len, dtype=np.int32)
        H, V1 = int(self.cfg.hidden_size), int(self.cfg.input_size) + 1
        if q.ndim != 2 or q.shape[1] != H or z.shape != (q.shape[0], V1):
            raise ValueError('queries must be [n, %d] and logits [n, %d], got %r and %r' % (H, V1, q.shape, z.shape))
        n = q.shape[0]
        if k.ndim != 3 or k.shape[0] != n or k.shape[2] != H or v.shape != k.shape[:2] or ln.shape != (n,):
            raise ValueError('self_keys must be [n, S, %d], self_values [n, S] and self_len [n], got %r, %r and %r' % (H, k.shape, v.shape, ln.shape))
        g = self._group(group, n)
        cc, sc = self.cache_gen_config(theta, lam), self.cache_self_config(window)
        out = dict(cache_prob=np.empty((n, V1), np.float32), logprob=np.empty((n, V1), np.float32), lse=np.empty(n, np.float32))
        self._ck(self._lib.fsmg_cache_self_distribution(self._h, cache._ptr() if cache is not None else None, C.byref(cc), C.byref(sc), n,
                                                        _f32p(q), _f32p(z), _f32p(k), v.ctypes.data_as(_I32P), ln.ctypes.data_as(_I32P),
                                                        k.shape[1], g.ctypes.data_as(_I32P) if g is not None else None,
                                                        _f32p(out['cache_prob']), _f32p(out['logprob']), _f32p(out['lse'])))
        return out

    # -- dynamic evaluation (include/fsmg.h "dynamic evaluation") --------------------------------------------------
    @staticmethod
    def dyneval_config(rule='sgd', seg_len=1, rows_per_step=1, lr=0.0, decay=0.0, eps=1e-3, clip_norm=0.0, adapt_reported=True):
        """the fsmg_dyneval_config struct; rule: 'sgd' / 'rms' (or the enum value)"""
        if rule not in DYNEVAL_RULES and rule not in DYNEVAL_RULES.values():
            raise ValueError("rule must be 'sgd' or 'rms', got %r" % (rule,))
        return FsmgDynevalConfig(struct_size=C.sizeof(FsmgDynevalConfig), rule=DYNEVAL_RULES.get(rule, rule), seg_len=int(seg_len),
                                 rows_per_step=int(rows_per_step), lr=float(lr), decay=float(decay), eps=float(eps),
                                 clip_norm=float(clip_norm), adapt_reported=int(bool(adapt_reported)), reserved=0)

    def _dyn_cfg(self, cfg):
        return cfg if isinstance(cfg, FsmgDynevalConfig) else self.dyneval_config(**cfg)

    @staticmethod
    def _opt_len(lengths, count):
        """optional host lengths of `count` rows -> (pointer or None, keepalive)"""
        if lengths is None:
            return None, None
        a = np.ascontiguousarray(lengths, dtype=np.int32).reshape(-1)
        if a.size != count:
            raise ValueError('%d lengths for %d sequences' % (a.size, count))
        return C.c_void_p(a.ctypes.data), a

    def dyneval_stats_reset(self):
        self._ck(self._lib.fsmg_dyneval_stats_reset(self._h))

    def dyneval_stats_accumulate(self):
        """ms_sum += g * g of the gradient the last forward_backward* left; count += 1"""
        self._ck(self._lib.fsmg_dyneval_stats_accumulate(self._h))

    def dyneval_stats_info(self):
        """-> (count, mean_rms)"""
        count, mean = C.c_int64(), C.c_float()
        self._ck(self._lib.fsmg_dyneval_stats_info(self._h, C.byref(count), C.byref(mean)))
        return int(count.value), float(mean.value)

    def dyneval_stats_get(self, name):
        out = np.empty(self._shape(name), np.float32)
        self._ck(self._lib.fsmg_dyneval_stats_get(self._h, name.encode(), _f32p(out), out.size))
        return out

    def dyneval_stats_set(self, name, value):
        a = np.ascontiguousarray(value, dtype=np.float32)
        self._ck(self._lib.fsmg_dyneval_stats_set(self._h, name.encode(), _f32p(a), a.size))

    def dyneval_stats_set_count(self, count):
        self._ck(self._lib.fsmg_dyneval_stats_set_count(self._h, int(count)))

    def dyneval_score(self, cfg, tokens, lengths=None, first_reported=0):
        """one stream: tokens int32 [R, max_len], lengths int32 [R] or None, rows [first_reported, R) reported
        -> dict(logprob float32 [R, max_len], row_nll float32 [R], nll float)"""
        c = self._dyn_cfg(cfg)
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        if t.ndim != 2 or t.shape[1] != self.max_len:
            raise ValueError('tokens %r do not match [R, max_len=%d]' % (t.shape, self.max_len))
        lp_, _keep = self._opt_len(lengths, t.shape[0])
        lp = np.empty(t.shape, np.float32)
        row = np.empty(t.shape[0], np.float32)
        nll = C.c_float()
        self._ck(self._lib.fsmg_dyneval_score(self._h, C.byref(c), C.c_void_p(t.ctypes.data), lp_, t.shape[0], int(first_reported),
                                              _f32p(lp), _f32p(row), C.byref(nll)))
        return dict(logprob=lp, row_nll=row, nll=float(nll.value))

    def dyneval_eval_step(self, cfg, support, query, support_len=None, query_len=None):
        """support [N,K,T], query [N,Q,T] int32, optional lengths [N,K] / [N,Q] -> the NLL over all artists' scored query positions"""
        c = self._dyn_cfg(cfg)
        n, k, q = self._episode_shape(support, query, None)
        s = np.ascontiguousarray(support, dtype=np.int32)
        qq = np.ascontiguousarray(query, dtype=np.int32)
        sl, _k1 = self._opt_len(support_len, n * k)
        ql, _k2 = self._opt_len(query_len, n * q)
        nll = C.c_float()
        self._ck(self._lib.fsmg_dyneval_eval_step(self._h, C.byref(c), C.c_void_p(s.ctypes.data), C.c_void_p(qq.ctypes.data), sl, ql,
                                                  n, k, q, C.byref(nll)))
        return float(nll.value)

    def dyneval_generate(self, cfg, support, num, support_len=None, n_seq=1, temperature=1.0, top_k=0, seed=0, primer=None,
                         logprobs=False, top_p=0.0, min_p=0.0, repetition_penalty=1.0, repeat_window=0):
        """adapt on the support stream [rows, max_len] by dynamic evaluation, generate at theta_l, restore theta"""
        c = self._dyn_cfg(cfg)
        s = np.ascontiguousarray(support, dtype=np.int32).reshape(-1, self.max_len)
        sl, _k1 = self._opt_len(support_len, s.shape[0])
        g, pp, _keep = self._gen_args(n_seq, num, temperature, top_k, seed, primer)
        f = self.gen_filters(top_p, min_p, repetition_penalty, repeat_window)
        toks = np.empty((int(n_seq), int(num)), np.int32)
        lp = np.empty((int(n_seq), int(num)), np.float32) if logprobs else None
        self._ck(self._lib.fsmg_dyneval_generate(self._h, C.byref(c), C.c_void_p(s.ctypes.data), sl, s.shape[0], C.byref(g),
                                                 C.byref(f) if f is not None else None, pp, toks.ctypes.data_as(_I32P),
                                                 _f32p(lp) if logprobs else None))
        return (toks, lp) if logprobs else toks

    def read_losses(self, n):
        out = np.empty(n, np.float32)
        self._ck(self._lib.fsmg_read_losses(self._h, _f32p(out), n))
        return out

    def stats(self):
        st = FsmgStats()
        self._ck(self._lib.fsmg_get_stats(self._h, C.byref(st)))
        return {name: int(getattr(st, name)) for name, _ in FsmgStats._fields_}

    def synchronize(self):
        self._ck(self._lib.fsmg_synchronize(self._h))

    # -- introspection ---------------------------------------------------------------------
    def debug_dims(self):
        d = (C.c_int32 * 5)()
        self._ck(self._lib.fsmg_debug_dims(self._h, d))
        return dict(Ep=d[0], Hp=d[1], V1p=d[2], B=d[3], T=d[4])

    # -- dropout of the train passes (include/fsmg.h "Dropout") -----------------------------------------------------
    @staticmethod
    def dropout_config(keep_input=1.0, keep_output=1.0, variational=False, seed=0):
        """the fsmg_dropout_config struct"""
        return FsmgDropoutConfig(struct_size=C.sizeof(FsmgDropoutConfig), keep_input=float(keep_input), keep_output=float(keep_output),
                                 variational=int(variational), seed=int(seed) & 0xFFFFFFFFFFFFFFFF)

    def dropout_enable(self, cfg=None, **kw):
        """the gradient passes of the train forms are dropped from here on; cfg: FsmgDropoutConfig, a dict of dropout_config's keywords, or keywords"""
        c = cfg if isinstance(cfg, FsmgDropoutConfig) else self.dropout_config(**dict(cfg or {}, **kw))
        self._ck(self._lib.fsmg_dropout_enable(self._h, C.byref(c)))

    def dropout_disable(self):
        self._ck(self._lib.fsmg_dropout_disable(self._h))

    def dropout_info(self):
        """-> dict(enabled, last_pass (-1: none yet), next_pass, bytes)"""
        out = (C.c_int64 * 4)()
        self._ck(self._lib.fsmg_dropout_info(self._h, out))
        return dict(enabled=bool(out[0]), last_pass=int(out[1]), next_pass=int(out[2]), bytes=int(out[3]))

    def dropout_set_pass(self, next_pass):
        self._ck(self._lib.fsmg_dropout_set_pass(self._h, int(next_pass)))

    def dropout_mask(self, pass_index, site, B):
        """-> uint8 [T, B, width]: the 0 / 1 mask of `site` in pass `pass_index` for B sequences (device row order t * B + b)"""
        W = self.cfg.embedding_size if site == 0 else self.cfg.hidden_size
        out = np.zeros((self.max_len, max(int(B), 1), W), np.uint8)        # (a bad site / B: the library refuses before it writes)
        self._ck(self._lib.fsmg_dropout_mask(self._h, int(pass_index), int(site), int(B), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def dropout_read(self, site, B=None):
        """-> float32 [T, B, Ep or Hp]: the masked activations of the last dropped pass at `site` (pads included)"""
        d = self.debug_dims()
        B = d['B'] if B is None else int(B)
        ld = d['Ep'] if site == 0 else d['Hp']
        return self.debug_read('drop%d' % site, d['T'] * B * ld).reshape(d['T'], B, ld)

    # -- Meta-SGD: learned per-parameter inner rates (include/fsmg.h "Meta-SGD") ------------------------------------
    @staticmethod
    def msgd_config(alpha_init=1.0, alpha_lr=0.0, alpha_min=0.0, alpha_max=float('inf'), alpha_clip_norm=0.0):
        """the fsmg_msgd_config struct"""
        return FsmgMsgdConfig(struct_size=C.sizeof(FsmgMsgdConfig), alpha_init=float(alpha_init), alpha_lr=float(alpha_lr),
                              alpha_min=float(alpha_min), alpha_max=float(alpha_max), alpha_clip_norm=float(alpha_clip_norm), reserved=0)

    def msgd_enable(self, cfg=None, **kw):
        """every adaptation of this handle takes the rates from here on; cfg: FsmgMsgdConfig, a dict of msgd_config's keywords, or keywords"""
        c = cfg if isinstance(cfg, FsmgMsgdConfig) else self.msgd_config(**dict(cfg or {}, **kw))
        self._ck(self._lib.fsmg_msgd_enable(self._h, C.byref(c)))

    def msgd_disable(self):
        self._ck(self._lib.fsmg_msgd_disable(self._h))

    def msgd_info(self):
        """-> dict(enabled, allocated, count, pending)"""
        out = (C.c_int64 * 4)()
        self._ck(self._lib.fsmg_msgd_info(self._h, out))
        return dict(enabled=bool(out[0]), allocated=bool(out[1]), count=int(out[2]), pending=bool(out[3]))

    def msgd_fill(self, value):
        """A = value everywhere, Adam slots of the rates zero"""
        self._ck(self._lib.fsmg_msgd_fill(self._h, float(value)))

    def msgd_get_alpha(self, name):
        out = np.empty(self._shape(name), np.float32)
        self._ck(self._lib.fsmg_msgd_get_alpha(self._h, name.encode(), _f32p(out), out.size))
        return out

    def msgd_set_alpha(self, name, value):
        a = np.ascontiguousarray(value, dtype=np.float32)
        self._ck(self._lib.fsmg_msgd_set_alpha(self._h, name.encode(), _f32p(a), a.size))

    def msgd_get_alphas(self):
        return {k: self.msgd_get_alpha(k) for k in self.param_shapes}

    def msgd_get_opt_state(self, name):
        m = np.empty(self._shape(name), np.float32)
        v = np.empty(self._shape(name), np.float32)
        self._ck(self._lib.fsmg_msgd_get_opt_state(self._h, name.encode(), _f32p(m), _f32p(v), m.size))
        return m, v

    def msgd_set_opt_state(self, name, m, v):
        m = np.ascontiguousarray(m, dtype=np.float32)
        v = np.ascontiguousarray(v, dtype=np.float32)
        self._ck(self._lib.fsmg_msgd_set_opt_state(self._h, name.encode(), _f32p(m), _f32p(v), m.size))

    def msgd_get_grad(self, name):
        """GA of the pending rate gradient (a maml_forward_backward* on an enabled handle, before apply_update)"""
        out = np.empty(self._shape(name), np.float32)
        self._ck(self._lib.fsmg_msgd_get_grad(self._h, name.encode(), _f32p(out), out.size))
        return out

    def msgd_grad_buffer(self):
        """-> (device pointer, float count) of GA: what a data-parallel wrapper all-reduces next to grad_buffer()"""
        ptr, count = _P(), C.c_int64()
        self._ck(self._lib.fsmg_msgd_grad_buffer(self._h, C.byref(ptr), C.byref(count)))
        return ptr.value, count.value

    def msgd_get_sum(self, name):
        """S of the last train-form adaptation, shaped like get_param(name)"""
        shape = self._shape(name)
        return self.debug_read('msgd_sum:' + name, int(np.prod(shape))).reshape(shape)

    # -- learned optimiser: a meta-learner LSTM cell per element (include/fsmg.h "learned optimiser") ----------------
    LOPT_NPHI = 14                      # wF[6], bF, wI[6], bI

    @staticmethod
    def lopt_config(bF_init=6.0, bI_init=0.0, gate_scale=2.0, phi_lr=0.0, phi_clip_norm=0.0, max_train_steps=4):
        """the fsmg_lopt_config struct"""
        return FsmgLoptConfig(struct_size=C.sizeof(FsmgLoptConfig), bF_init=float(bF_init), bI_init=float(bI_init), gate_scale=float(gate_scale),
                              phi_lr=float(phi_lr), phi_clip_norm=float(phi_clip_norm), max_train_steps=int(max_train_steps), reserved=0)

    def lopt_enable(self, cfg=None, **kw):
        """every adaptation of this handle takes the learned rule from here on; cfg: FsmgLoptConfig, a dict of lopt_config's keywords, or keywords"""
        c = cfg if isinstance(cfg, FsmgLoptConfig) else self.lopt_config(**dict(cfg or {}, **kw))
        self._ck(self._lib.fsmg_lopt_enable(self._h, C.byref(c)))

    def lopt_disable(self):
        self._ck(self._lib.fsmg_lopt_disable(self._h))

    def lopt_info(self):
        """-> dict(enabled, allocated, max_train_steps, pending)"""
        out = (C.c_int64 * 4)()
        self._ck(self._lib.fsmg_lopt_info(self._h, out))
        return dict(enabled=bool(out[0]), allocated=bool(out[1]), max_train_steps=int(out[2]), pending=bool(out[3]))

    def lopt_get_phi(self):
        """-> float32 [14]: wF[6], bF, wI[6], bI"""
        out = np.empty(self.LOPT_NPHI, np.float32)
        self._ck(self._lib.fsmg_lopt_get_phi(self._h, _f32p(out)))
        return out

    def _phi14(self, value):
        a = np.ascontiguousarray(value, dtype=np.float32).reshape(-1)
        if a.size != self.LOPT_NPHI:
            raise ValueError('Phi holds %d floats, got %d' % (self.LOPT_NPHI, a.size))
        return a

    def lopt_set_phi(self, phi):
        a = self._phi14(phi)
        self._ck(self._lib.fsmg_lopt_set_phi(self._h, _f32p(a)))

    def lopt_get_opt_state(self):
        m, v = np.empty(self.LOPT_NPHI, np.float32), np.empty(self.LOPT_NPHI, np.float32)
        self._ck(self._lib.fsmg_lopt_get_opt_state(self._h, _f32p(m), _f32p(v)))
        return m, v

    def lopt_set_opt_state(self, m, v):
        m, v = self._phi14(m), self._phi14(v)
        self._ck(self._lib.fsmg_lopt_set_opt_state(self._h, _f32p(m), _f32p(v)))

    def lopt_get_grad(self):
        """GPhi of the pending gradient (a train form of maml_* on an enabled handle, before apply_update)"""
        out = np.empty(self.LOPT_NPHI, np.float32)
        self._ck(self._lib.fsmg_lopt_get_grad(self._h, _f32p(out)))
        return out

    def lopt_grad_buffer(self):
        """-> (device pointer, 14) of GPhi: what a data-parallel wrapper all-reduces next to grad_buffer()"""
        ptr, count = _P(), C.c_int64()
        self._ck(self._lib.fsmg_lopt_grad_buffer(self._h, C.byref(ptr), C.byref(count)))
        return ptr.value, count.value

    def lopt_get_gates(self, name):
        """-> (F, I) after the last inner step, shaped like get_param(name)"""
        shape = self._shape(name)
        n = int(np.prod(shape))
        return self.debug_read('lopt_F:' + name, n).reshape(shape), self.debug_read('lopt_I:' + name, n).reshape(shape)

    def lopt_get_stored(self, t, name):
        """the support gradient a train form stored for inner step t (from 0), shaped like get_param(name)"""
        shape = self._shape(name)
        return self.debug_read('lopt_g%d:%s' % (int(t), name), int(np.prod(shape))).reshape(shape)

    def lopt_get_scalars(self):
        """-> (step_t[8], L_t[8]) of the last train-form adaptation"""
        sc = self.debug_read('lopt_scalars', 16)
        return sc[:8].copy(), sc[8:].copy()

    def lopt_get_replayed(self, name):
        """theta_K as the back-propagation replayed it; needs debug_set('keep_adapted', 1) before the train form"""
        shape = self._shape(name)
        return self.debug_read('lopt_theta:' + name, int(np.prod(shape))).reshape(shape)

    def debug_set(self, what, value):
        """run-time knob of the handle (include/fsmg.h: chain_spin_limit, fallback_steps, persistent, eager, inplace_dlogits,
        upd_split, upd_defer, xov_dk_tail, xov_selfcheck, xov_selfcheck_fault, keep_adapted)"""
        self._ck(self._lib.fsmg_debug_set(self._h, what.encode(), int(value)))

    def clock_begin(self, microseconds):
        """start the shader-clock probe (its own stream); issue the work to be measured next, then clock_end()"""
        self._ck(self._lib.fsmg_debug_clock_begin(self._h, int(microseconds)))

    def clock_end(self):
        ghz = C.c_float()
        self._ck(self._lib.fsmg_debug_clock_end(self._h, C.byref(ghz)))
        return float(ghz.value)

    def debug_read(self, what, count):
        out = np.empty(int(count), np.float32)
        self._ck(self._lib.fsmg_debug_read(self._h, what.encode(), _f32p(out), out.size))
        return out

    def get_adapted(self, name):
        """theta' of the last MAML-style call, shaped like get_param(name); needs debug_set('keep_adapted', 1) before that call"""
        shape = self._shape(name)
        return self.debug_read('adapted:' + name, int(np.prod(shape))).reshape(shape)

    def step_profile(self, which):
        """-> uint64 [n_blocks, n_waves, 8] s_memtime stamps of one instrumented recurrent step kernel"""
        buf = np.zeros(1 << 20, np.uint64)
        nb, nw = C.c_int32(), C.c_int32()
        self._ck(self._lib.fsmg_debug_step_profile(self._h, int(which), buf.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                   buf.size, C.byref(nb), C.byref(nw)))
        return buf[:nb.value * nw.value * 8].reshape(nb.value, nw.value, 8)

    def timing_enable(self, on=True):
        self._ck(self._lib.fsmg_timing_enable(self._h, int(bool(on))))

    def timing_select(self, kernel_class=None):
        self._ck(self._lib.fsmg_timing_select(self._h, kernel_class.encode() if kernel_class else None))

    def timing_reset(self):
        self._ck(self._lib.fsmg_timing_reset(self._h))

    def timing_read(self, kernel_class):
        ms, n = C.c_double(), C.c_int64()
        self._ck(self._lib.fsmg_timing_read(self._h, kernel_class.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value


class FsmgUnigram(object):
    """Device-resident unigram counts (include/fsmg.h fsmg_unigram_*): the graph of the reference's UnigramModel
    (/root/reference/src/models/unigram_model.py:26-39) -- scatter_add histogram, gather / reduce_sum, -mean(log)."""

    def __init__(self, input_size, device=0):
        self._lib = load_library()
        self.input_size = int(input_size)
        handle = _P()
        rc = self._lib.fsmg_unigram_create(self.input_size, int(device), C.byref(handle))
        if rc != 0:
            raise FsmgError(rc, self._lib.fsmg_unigram_last_error(None).decode())
        self._h = handle

    def _ck(self, rc):
        if rc != 0:
            raise FsmgError(rc, self._lib.fsmg_unigram_last_error(self._h).decode())

    def close(self):
        if getattr(self, '_h', None):
            self._lib.fsmg_unigram_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _words(words):
        if isinstance(words, tuple):                  # (device address, count)
            return C.c_void_p(int(words[0])), int(words[1]), 1, None
        a = np.ascontiguousarray(words, dtype=np.int32).ravel()
        return C.c_void_p(a.ctypes.data), a.size, 0, a

    def nll(self, words):
        ptr, n, dev, keep = self._words(words)
        out = C.c_float()
        self._ck(self._lib.fsmg_unigram_nll(self._h, ptr, n, dev, C.byref(out)))
        return float(out.value)

    def train(self, words, want_loss=True):
        ptr, n, dev, keep = self._words(words)
        out = C.c_float()
        self._ck(self._lib.fsmg_unigram_train(self._h, ptr, n, dev, C.byref(out) if want_loss else None))
        return float(out.value) if want_loss else None

    def get_counts(self):
        out = np.empty(self.input_size, np.float32)
        self._ck(self._lib.fsmg_unigram_get_counts(self._h, _f32p(out), out.size))
        return out

    def set_counts(self, counts):
        a = np.ascontiguousarray(counts, dtype=np.float32)
        if a.size != self.input_size:
            raise ValueError('counts must have input_size entries')
        self._ck(self._lib.fsmg_unigram_set_counts(self._h, _f32p(a), a.size))

    def argmax(self):
        w = C.c_int32()
        self._ck(self._lib.fsmg_unigram_argmax(self._h, C.byref(w)))
        return int(w.value)
