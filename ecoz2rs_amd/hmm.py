"""Host-side mirror of the reference's HMM wrappers.

``hmm_learn`` / ``hmm_classify_sequences`` / ``hmm_classify_predictors`` / ``hmm_show`` / ``set_random_seed`` take the
arguments of the Rust functions of the same name (/root/reference/src/ecoz2_lib/mod.rs:188-190, 385-494) and call the
same C symbols; the array-level functions drive the same HIP kernels without files (tests, bench).
"""
import contextlib
import ctypes as C
import math
import os
from types import SimpleNamespace

import numpy as np

from ._lib import c_char_pp, check, lib

HMM_LEARN_CALLBACK = C.CFUNCTYPE(None, C.c_char_p, C.c_double)
_dpp = C.POINTER(C.c_void_p)


def _sig(name, restype, *argtypes):
    fn = getattr(lib, name)
    fn.restype = restype
    fn.argtypes = list(argtypes)
    return fn


_sig("ecoz2_set_random_seed", C.c_ulong, C.c_long)
_sig("ecoz2_hmm_learn", C.c_int, C.c_int, C.c_int, c_char_pp, C.c_uint, C.c_double, C.c_double, C.c_int, C.c_int,
     HMM_LEARN_CALLBACK)
_sig("ecoz2_hmm_classify", C.c_int, c_char_pp, C.c_uint, c_char_pp, C.c_uint, C.c_int, C.c_char_p)
_sig("ecoz2_hmm_classify_predictors", C.c_int, c_char_pp, C.c_uint, c_char_pp, C.c_int, c_char_pp, C.c_int, C.c_int,
     C.c_char_p)
_sig("ecoz2_hmm_show", C.c_int, C.c_char_p, C.c_char_p)
_sig("e2vq_hmm_init", C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("e2vq_hmm_save", C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("e2vq_hmm_info", C.c_int, C.c_char_p, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int))
_sig("e2vq_hmm_load", C.c_int, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("e2vq_hmm_score", C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, _dpp, _dpp, _dpp, C.c_void_p, C.c_void_p,
     C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("e2vq_hmm_acc_words", C.c_int64, C.c_int, C.c_int)
_sig("e2vq_hmm_estep", C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("ecoz2_seq_show_files", C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, c_char_pp, C.c_int)
_sig("e2vq_seq_show_files", C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, c_char_pp, C.c_int, C.c_int, C.c_int)
_sig("e2vq_hmm_viterbi", C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("e2vq_hmm_train", C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int))
_sig("e2vq_hmm_learn_classes", C.c_int, C.c_int, C.c_int, c_char_pp, C.c_uint, C.c_double, C.c_double, C.c_int,
     HMM_LEARN_CALLBACK)
_sig("e2vq_hmm_train_classes", C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_void_p)
_sig("e2vq_hmm_learn_grid", C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, c_char_pp, C.c_uint, C.c_double, C.c_double,
     C.c_int, HMM_LEARN_CALLBACK)
_sig("e2vq_hmm_train_grid", C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_void_p)
_sig("e2vq_hmm_classify_grid", C.c_int, c_char_pp, C.c_uint, c_char_pp, C.c_uint, C.c_int, C.c_char_p, C.c_char_p)
_sig("e2vq_hmm_score_grid", C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("e2vq_hmm_scan_windows", C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p)
_sig("e2vq_hmm_scan", C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, _dpp, _dpp, _dpp, C.c_void_p, C.c_void_p,
     C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_int)
_sig("e2vq_hmm_scan_last_kernel_ms", C.c_int, C.POINTER(C.c_float))
_sig("e2vq_hmm_scan_files", C.c_int, c_char_pp, C.c_uint, C.c_char_p, c_char_pp, C.c_int, C.c_int, C.c_int, C.c_int,
     C.c_int64, C.c_int64, C.c_double, C.c_char_p)
_sig("e2vq_hmm_scan_report", C.c_int, C.c_char_p, C.c_int64, C.c_int, c_char_pp, C.c_int64, C.c_int64, C.c_int64, C.c_int,
     C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_char_p)

_sig("e2vq_hmm_segment", C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, _dpp, _dpp, _dpp, C.c_void_p, C.c_void_p,
     C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int)
_sig("e2vq_hmm_segment_last_kernel_ms", C.c_int, C.POINTER(C.c_float))
_sig("e2vq_hmm_segment_files", C.c_int, c_char_pp, C.c_uint, C.c_char_p, c_char_pp, C.c_int, C.c_int, C.c_int, C.c_int,
     C.c_double, C.c_char_p)
_sig("e2vq_hmm_segment_report", C.c_int, C.c_char_p, C.c_int64, C.c_int, c_char_pp, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_double, C.c_double, C.c_char_p)
_sig("e2vq_hmm_segment_posteriors", C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, _dpp, _dpp, _dpp, C.c_void_p,
     C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int)
_sig("e2vq_hmm_segment_posteriors_last_kernel_ms", C.c_int, C.POINTER(C.c_float))
_sig("e2vq_hmm_segment_files_posteriors", C.c_int, c_char_pp, C.c_uint, C.c_char_p, c_char_pp, C.c_int, C.c_int, C.c_int,
     C.c_int, C.c_double, C.c_char_p, C.c_char_p)
_sig("e2vq_hmm_segment_report_posteriors", C.c_int, C.c_char_p, C.c_int64, C.c_int, c_char_pp, C.c_int, C.c_int, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_char_p, C.c_char_p)
_sig("e2vq_hmm_segment_trans", C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, _dpp, _dpp, _dpp, C.c_void_p,
     C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int)
_sig("e2vq_hmm_segment_trans_last_kernel_ms", C.c_int, C.POINTER(C.c_float))
_sig("e2vq_hmm_segment_trans_files", C.c_int, c_char_pp, C.c_uint, C.c_char_p, c_char_pp, C.c_int, C.c_int, C.c_int, C.c_int,
     C.c_double, C.c_char_p, C.c_char_p)
_sig("e2vq_hmm_segment_trans_report", C.c_int, C.c_char_p, C.c_int64, C.c_int, c_char_pp, C.c_int, C.c_int, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_char_p)
_sig("e2vq_hmm_segment_trans_posteriors", C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, _dpp, _dpp, _dpp, C.c_void_p,
     C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int)
_sig("e2vq_hmm_segment_trans_posteriors_last_kernel_ms", C.c_int, C.POINTER(C.c_float))
_sig("e2vq_hmm_segment_trans_files_posteriors", C.c_int, c_char_pp, C.c_uint, C.c_char_p, c_char_pp, C.c_int, C.c_int, C.c_int,
     C.c_int, C.c_double, C.c_char_p, C.c_char_p, C.c_char_p)
_sig("e2vq_hmm_transitions_read", C.c_int, C.c_char_p, C.c_int, c_char_pp, C.c_void_p)
_sig("e2vq_hmm_transitions_write", C.c_int, C.c_char_p, C.c_int, c_char_pp, C.c_void_p)
_sig("e2vq_hmm_class_transitions", C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p)
_sig("e2vq_hmm_transitions_files", C.c_int, c_char_pp, C.c_uint, c_char_pp, C.c_int, C.c_double, C.c_char_p)
_sig("e2vq_hmm_transitions_acc_words", C.c_int64, C.c_int)
_sig("e2vq_hmm_transitions_estep", C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, _dpp, _dpp, _dpp, C.c_void_p, C.c_void_p,
     C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int)
_sig("e2vq_hmm_transitions_estep_last_kernel_ms", C.c_int, C.POINTER(C.c_float))
_sig("e2vq_hmm_train_transitions", C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, _dpp, _dpp, _dpp, C.c_void_p, C.c_void_p,
     C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), HMM_LEARN_CALLBACK,
     C.c_int)
_sig("e2vq_hmm_learn_transitions_files", C.c_int, c_char_pp, C.c_uint, C.c_char_p, c_char_pp, C.c_int, C.c_int, C.c_int, C.c_int,
     C.c_double, C.c_char_p, C.c_double, C.c_double, C.c_int, C.c_char_p)
_sig("e2vq_hmm_loop_estep", C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, _dpp, _dpp, _dpp, C.c_void_p, C.c_void_p,
     C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int)
_sig("e2vq_hmm_loop_estep_last_kernel_ms", C.c_int, C.POINTER(C.c_float))
_sig("e2vq_hmm_train_loop", C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, _dpp, _dpp, _dpp, C.c_void_p, C.c_void_p,
     C.c_int, C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_int,
     C.POINTER(C.c_int), HMM_LEARN_CALLBACK, C.c_int)
_sig("e2vq_hmm_learn_loop_files", C.c_int, c_char_pp, C.c_uint, C.c_char_p, c_char_pp, C.c_int, C.c_int, C.c_int, C.c_int,
     C.c_double, C.c_char_p, C.c_int, c_char_pp, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_char_p, HMM_LEARN_CALLBACK)

_sig("e2vq_hmm_segment_stream_open", C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, _dpp, _dpp, _dpp, C.c_double,
     C.POINTER(C.c_void_p))
_sig("e2vq_hmm_segment_stream_feed", C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_int64))
_sig("e2vq_hmm_segment_stream_flush", C.c_int, C.c_void_p, C.POINTER(C.c_int64))
_sig("e2vq_hmm_segment_stream_close", C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int64))
_sig("e2vq_hmm_segment_stream_take", C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
     C.POINTER(C.c_int64), C.POINTER(C.c_int64))
_sig("e2vq_hmm_segment_stream_kernel_ms", C.c_int, C.c_void_p, C.POINTER(C.c_float))
_sig("e2vq_hmm_segment_stream_stats", C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_float))
_sig("e2vq_hmm_segment_stream_free", None, C.c_void_p)
_sig("e2vq_hmm_segment_continuous_files", C.c_int, c_char_pp, C.c_uint, C.c_char_p, c_char_pp, C.c_int, C.c_int, C.c_int, C.c_int,
     C.c_double, C.c_char_p, C.c_char_p)
_sig("e2vq_hmm_segment_trans_stream_open", C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, _dpp, _dpp, _dpp, C.c_void_p,
     C.POINTER(C.c_void_p))
_sig("e2vq_hmm_segment_trans_continuous_files", C.c_int, c_char_pp, C.c_uint, C.c_char_p, c_char_pp, C.c_int, C.c_int, C.c_int,
     C.c_int, C.c_double, C.c_char_p, C.c_char_p, C.c_char_p)
_sig("e2vq_hmm_posterior_stream_open", C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, _dpp, _dpp, _dpp, C.c_double,
     C.c_int64, C.c_int64, C.POINTER(C.c_void_p))
_sig("e2vq_hmm_posterior_stream_feed", C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_int64))
_sig("e2vq_hmm_posterior_stream_close", C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int64))
_sig("e2vq_hmm_posterior_stream_take", C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64))
_sig("e2vq_hmm_posterior_stream_kernel_ms", C.c_int, C.c_void_p, C.POINTER(C.c_float))
_sig("e2vq_hmm_posterior_stream_stats", C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
     C.POINTER(C.c_int64))
_sig("e2vq_hmm_posterior_stream_free", None, C.c_void_p)
_sig("e2vq_hmm_segment_continuous_files_posteriors", C.c_int, c_char_pp, C.c_uint, C.c_char_p, c_char_pp, C.c_int, C.c_int, C.c_int,
     C.c_int, C.c_double, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int64, C.c_int64)
_sig("e2vq_hmm_align", C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, _dpp, _dpp, _dpp, C.c_void_p, C.c_void_p, C.c_int,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_int)
_sig("e2vq_hmm_align_last_kernel_ms", C.c_int, C.POINTER(C.c_float))
_sig("e2vq_hmm_align_report", C.c_int, C.c_char_p, C.c_int64, C.c_int, c_char_pp, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_char_p)
_sig("e2vq_hmm_align_files", C.c_int, c_char_pp, C.c_uint, C.c_char_p, c_char_pp, c_char_pp, C.c_int, C.c_int, C.c_int, C.c_int,
     C.c_double, C.c_char_p, C.c_char_p)
_sig("e2vq_hmm_align_posteriors", C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, _dpp, _dpp, _dpp, C.c_void_p, C.c_void_p,
     C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_int)
_sig("e2vq_hmm_align_posteriors_last_kernel_ms", C.c_int, C.POINTER(C.c_float))
_sig("e2vq_hmm_align_unit_moments", C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p)
_sig("e2vq_hmm_align_report_posteriors", C.c_int, C.c_char_p, C.c_int64, C.c_int, c_char_pp, C.c_int, C.c_int, C.c_int, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p)
_sig("e2vq_hmm_align_files_posteriors", C.c_int, c_char_pp, C.c_uint, C.c_char_p, c_char_pp, c_char_pp, C.c_int, C.c_int, C.c_int,
     C.c_int, C.c_double, C.c_char_p, C.c_char_p, C.c_char_p)
_sig("e2vq_hmm_embedded_estep", C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, _dpp, _dpp, _dpp, C.c_void_p, C.c_void_p,
     C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, _dpp, C.c_void_p, C.c_void_p, C.c_int)
_sig("e2vq_hmm_train_embedded", C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, _dpp, _dpp, _dpp, C.c_void_p, C.c_void_p,
     C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_int,
     C.POINTER(C.c_int), C.c_int)
_sig("e2vq_hmm_embedded_last_kernel_ms", C.c_int, C.POINTER(C.c_float))
_sig("e2vq_hmm_learn_embedded_files", C.c_int, c_char_pp, C.c_uint, C.c_char_p, c_char_pp, c_char_pp, C.c_int, C.c_int, C.c_int,
     C.c_int, C.c_double, C.c_char_p, C.c_double, C.c_double, C.c_int, C.c_char_p, HMM_LEARN_CALLBACK)


def _strs(items):
    arr = (C.c_char_p * len(items))(*[str(p).encode() for p in items])
    return C.cast(arr, c_char_pp), arr


def _kernel_ms(fn):
    """what an e2vq_*_last_kernel_ms export gives: the HIP-event time of the calling thread's last call, in ms"""
    ms = C.c_float()
    check(fn(C.byref(ms)))
    return ms.value


@contextlib.contextmanager
def _body_env(name, body):
    """the variable `name` (ECOZ2_HMM_EMBED_BODY, ECOZ2_HMM_POSTERIOR_BODY, ECOZ2_HMM_SEGMENT_TRANS_BODY,
    ECOZ2_HMM_TRANS_FB_BODY, ECOZ2_HMM_ALIGN_POSTERIOR_BODY) = body ("auto", "resident" or "looped") for the
    duration of a call; None leaves the environment alone"""
    if body is None:
        yield
        return
    before = os.environ.get(name)
    os.environ[name] = str(body)
    try:
        yield
    finally:
        if before is None:
            del os.environ[name]
        else:
            os.environ[name] = before


def trans_fb_body(body):
    """a context in which ECOZ2_HMM_TRANS_FB_BODY = body ("auto", "resident" or "looped"; None leaves the environment alone):
    the kernel body of the forward-backward passes under class-to-class prices -- the looped one
    takes any number of wave-slots, auto picks it above 16, and the results are the same bit for bit.  It is what body= of
    `transitions_estep`, `train_transitions` and `learn_transitions_files` and grammar_posteriors_body= of `segment_files`
    enter; `segment_trans_posteriors` keeps its parameters and is called inside it:
        with hmm.trans_fb_body("auto"): hmm.segment_trans_posteriors(...)"""
    return _body_env("ECOZ2_HMM_TRANS_FB_BODY", body)


def set_random_seed(seed):
    """ecoz2_lib::set_random_seed (src/ecoz2_lib/mod.rs:188-190)"""
    return lib.ecoz2_set_random_seed(int(seed))


def hmm_learn(n, model_type, sequence_filenames, hmm_epsilon, val_auto, max_iterations, use_par=True, callback=None):
    """ecoz2_lib::hmm_learn (src/ecoz2_lib/mod.rs:385-419); callback(var: str, val: float) per E-step"""
    files, _k = _strs(sequence_filenames)
    cb = HMM_LEARN_CALLBACK((lambda v, x: callback(v.decode(), x)) if callback else (lambda _v, _x: None))
    check(lib.ecoz2_hmm_learn(int(n), int(model_type), files, len(sequence_filenames), float(hmm_epsilon),
                              float(val_auto), int(max_iterations), int(bool(use_par)), cb))


def hmm_learn_classes(n, model_type, sequence_filenames, hmm_epsilon, val_auto, max_iterations, callback=None):
    """`hmm learn --all-classes`: one model per class of the sequences, all trained together; per class
    the files and output of hmm_learn on that class's files after the same set_random_seed"""
    files, _k = _strs(sequence_filenames)
    cb = HMM_LEARN_CALLBACK((lambda v, x: callback(v.decode(), x)) if callback else (lambda _v, _x: None))
    check(lib.e2vq_hmm_learn_classes(int(n), int(model_type), files, len(sequence_filenames), float(hmm_epsilon),
                                     float(val_auto), int(max_iterations), cb))


def hmm_learn_grid(ns, model_type, sequence_filenames, hmm_epsilon, val_auto, max_iterations, callback=None):
    """`hmm learn --grid`: one model per (N in ns, M of the files, class at that M), all trained
    together; per grid point the files and output of hmm_learn_classes(N, ...) on the files of that M, for that class,
    after the same set_random_seed"""
    ns = [int(n) for n in ns]
    files, _k = _strs(sequence_filenames)
    cb = HMM_LEARN_CALLBACK((lambda v, x: callback(v.decode(), x)) if callback else (lambda _v, _x: None))
    check(lib.e2vq_hmm_learn_grid((C.c_int * max(len(ns), 1))(*ns), len(ns), int(model_type), files, len(sequence_filenames),
                                  float(hmm_epsilon), float(val_auto), int(max_iterations), cb))


def hmm_classify_sequences(model_filenames, sequence_filenames, show_ranked=False, classification_filename=None):
    """ecoz2_lib::hmm_classify_sequences (src/ecoz2_lib/mod.rs:421-447)"""
    m, _k1 = _strs(model_filenames)
    s, _k2 = _strs(sequence_filenames)
    check(lib.ecoz2_hmm_classify(m, len(model_filenames), s, len(sequence_filenames), int(show_ranked),
                                 str(classification_filename).encode() if classification_filename else None))


def hmm_classify_grid(model_filenames, sequence_filenames, show_ranked=False, classification_dir=None,
                      summary_filename=None):
    """`hmm classify --grid`: every (N, M) point of the given models classified in one batched scoring;
    per point the report (and CSV, as <classification_dir>/N<n>__M<m>.csv) of hmm_classify_sequences on that point's
    models and sequences, then the summary of the sweep (and its CSV)"""
    m, _k1 = _strs(model_filenames)
    s, _k2 = _strs(sequence_filenames)
    check(lib.e2vq_hmm_classify_grid(m, len(model_filenames), s, len(sequence_filenames), int(show_ranked),
                                     str(classification_dir).encode() if classification_dir else None,
                                     str(summary_filename).encode() if summary_filename else None))


def hmm_classify_predictors(model_filenames, cb_filenames, prd_filenames, show_ranked=False,
                            classification_filename=None):
    """ecoz2_lib::hmm_classify_predictors (src/ecoz2_lib/mod.rs:449-479)"""
    m, _k1 = _strs(model_filenames)
    c, _k2 = _strs(cb_filenames)
    p, _k3 = _strs(prd_filenames)
    check(lib.ecoz2_hmm_classify_predictors(m, len(model_filenames), c, len(cb_filenames), p, len(prd_filenames),
                                            int(show_ranked),
                                            str(classification_filename).encode() if classification_filename else None))


def hmm_show(hmm_filename, format="%Lg "):
    """ecoz2_lib::hmm_show (src/ecoz2_lib/mod.rs:481-494)"""
    check(lib.ecoz2_hmm_show(str(hmm_filename).encode(), format.encode()))


def seq_show_files(with_prob, gen_q_opt, no_sequence, hmm_filename, seq_filenames):
    """the reference's commented-out ecoz2_lib::seq_show_files (src/ecoz2_lib/mod.rs:496-528): `seq show -P / -Q`"""
    files, _k = _strs(seq_filenames)
    check(lib.ecoz2_seq_show_files(int(bool(with_prob)), int(bool(gen_q_opt)), int(bool(no_sequence)),
                                   str(hmm_filename).encode() if hmm_filename else b"", files, len(seq_filenames)))


# ---- array level ----------------------------------------------------------------------------------------------
def init_model(N, M, model_type):
    pi, A, B = np.zeros(N), np.zeros((N, N)), np.zeros((N, M))
    check(lib.e2vq_hmm_init(N, M, model_type, pi.ctypes.data, A.ctypes.data, B.ctypes.data))
    return pi, A, B


def save_model(path, class_name, pi, A, B):
    pi, A, B = (np.ascontiguousarray(x, dtype=np.float64) for x in (pi, A, B))
    check(lib.e2vq_hmm_save(str(path).encode(), class_name.encode(), len(pi), B.shape[1], pi.ctypes.data, A.ctypes.data,
                            B.ctypes.data))


def load_model(path):
    cls, N, M = C.create_string_buffer(96), C.c_int(), C.c_int()
    check(lib.e2vq_hmm_info(str(path).encode(), cls, C.byref(N), C.byref(M)))
    pi, A, B = np.zeros(N.value), np.zeros((N.value, N.value)), np.zeros((N.value, M.value))
    check(lib.e2vq_hmm_load(str(path).encode(), pi.ctypes.data, A.ctypes.data, B.ctypes.data))
    return cls.value.decode(), pi, A, B


def _pack(seqs):
    arrs = [np.ascontiguousarray(s, dtype=np.uint16) for s in seqs]
    offs = np.zeros(len(arrs) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(a) for a in arrs])
    sym = np.concatenate(arrs) if arrs and offs[-1] else np.zeros(0, dtype=np.uint16)
    return np.ascontiguousarray(sym), offs


def score(models, seqs, device=0):
    """models: list of (pi, A, B) sharing M; seqs: list of uint16 arrays -> dict of (S, K) arrays mant/exp2/status/log_prob"""
    K, S = len(models), len(seqs)
    ms = [tuple(np.ascontiguousarray(x, dtype=np.float64) for x in m) for m in models]
    Ns = (C.c_int * K)(*[len(m[0]) for m in ms])
    ptr = lambda i: (C.c_void_p * K)(*[m[i].ctypes.data for m in ms])
    sym, offs = _pack(seqs)
    mant, ex = np.zeros((S, K)), np.zeros((S, K), dtype=np.int64)
    st, lp = np.zeros((S, K), dtype=np.int32), np.zeros((S, K))
    check(lib.e2vq_hmm_score(device, K, Ns, ms[0][2].shape[1], ptr(0), ptr(1), ptr(2), sym.ctypes.data, offs.ctypes.data,
                             S, mant.ctypes.data, ex.ctypes.data, st.ctypes.data, lp.ctypes.data))
    return dict(mant=mant, exp2=ex, status=st, log_prob=lp)


def score_grid(models, seqs, ranges, device=0):
    """scores of K models of any (N, M) in one batch: models = [(pi, A, B)], seqs = [uint16 arrays]
    shared by all, ranges = [(lo, hi)] the sequences seqs[lo:hi] model k scores (ranges may overlap) -> per model a dict
    of (hi - lo,) arrays mant / exp2 / status / log_prob, each as `score` of that model on its slice"""
    K = len(models)
    if K != len(ranges):
        raise ValueError(f"{K} models for {len(ranges)} sequence ranges")
    ms = [tuple(np.asarray(x, dtype=np.float64) for x in m) for m in models]
    Ns = np.array([len(m[0]) for m in ms], dtype=np.int32)
    Ms = np.array([m[2].shape[1] if m[2].ndim == 2 else 0 for m in ms], dtype=np.int32)
    sizes = [m[0].size + m[1].size + m[2].size for m in ms]
    param_offs = np.zeros(K, dtype=np.int64)
    param_offs[1:] = np.cumsum(sizes)[:-1]
    params = np.ascontiguousarray(np.concatenate([np.concatenate([x.ravel() for x in m]) for m in ms]))
    sym, offs = _pack(seqs)
    lo = np.array([r[0] for r in ranges], dtype=np.int64)
    hi = np.array([r[1] for r in ranges], dtype=np.int64)
    out_offs = np.zeros(K, dtype=np.int64)
    out_offs[1:] = np.cumsum(np.maximum(hi - lo, 0))[:-1]
    n = max(int(np.maximum(hi - lo, 0).sum()), 1)
    mant, ex = np.zeros(n), np.zeros(n, dtype=np.int64)
    st, lp = np.zeros(n, dtype=np.int32), np.zeros(n)
    check(lib.e2vq_hmm_score_grid(device, K, Ns.ctypes.data, Ms.ctypes.data, params.ctypes.data, param_offs.ctypes.data,
                                  sym.ctypes.data, offs.ctypes.data, len(seqs), lo.ctypes.data, hi.ctypes.data,
                                  out_offs.ctypes.data, mant.ctypes.data, ex.ctypes.data, st.ctypes.data, lp.ctypes.data))
    return [dict(mant=mant[o:o + h - l].copy(), exp2=ex[o:o + h - l].copy(), status=st[o:o + h - l].copy(),
                 log_prob=lp[o:o + h - l].copy()) for o, l, h in zip(out_offs, lo, hi)]


def estep(pi, A, B, seqs, device=0):
    """one Baum-Welch E-step: (acc int64 words, mant, exp2, status)"""
    pi, A, B = (np.ascontiguousarray(x, dtype=np.float64) for x in (pi, A, B))
    N, M, S = len(pi), B.shape[1], len(seqs)
    sym, offs = _pack(seqs)
    acc = np.zeros(lib.e2vq_hmm_acc_words(N, M), dtype=np.int64)
    mant, ex, st = np.zeros(S), np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int32)
    check(lib.e2vq_hmm_estep(device, N, M, pi.ctypes.data, A.ctypes.data, B.ctypes.data, sym.ctypes.data, offs.ctypes.data,
                             S, acc.ctypes.data, mant.ctypes.data, ex.ctypes.data, st.ctypes.data))
    return acc, mant, ex, st


def train(pi, A, B, seqs, epsilon=1e-5, val_auto=0.3, max_iterations=-1, device=0):
    """Baum-Welch on arrays: -> (pi, A, B, [sum_log_prob per E-step])"""
    pi, A, B = (np.array(x, dtype=np.float64, copy=True) for x in (pi, A, B))
    N, M, S = len(pi), B.shape[1], len(seqs)
    sym, offs = _pack(seqs)
    hist, n = np.zeros(4096), C.c_int()
    check(lib.e2vq_hmm_train(device, N, M, pi.ctypes.data, A.ctypes.data, B.ctypes.data, sym.ctypes.data, offs.ctypes.data,
                             S, float(epsilon), float(val_auto), int(max_iterations), hist.ctypes.data, len(hist),
                             C.byref(n)))
    return pi, A, B, list(hist[:n.value])


def train_classes(models, class_seqs, epsilon=1e-5, val_auto=0.3, max_iterations=-1, device=0):
    """Baum-Welch of K classes in one batched training: models = [(pi, A, B)] sharing N and M,
    class_seqs = [[uint16 arrays] per class] -> [(pi, A, B, [sum_log_prob per E-step])], each as `train` on its class"""
    K = len(models)
    if K != len(class_seqs):
        raise ValueError(f"{K} models for {len(class_seqs)} classes")
    N, M = len(models[0][0]), np.asarray(models[0][2]).shape[1]
    pi = np.ascontiguousarray(np.stack([np.asarray(m[0], dtype=np.float64) for m in models]))
    A = np.ascontiguousarray(np.stack([np.asarray(m[1], dtype=np.float64) for m in models]))
    B = np.ascontiguousarray(np.stack([np.asarray(m[2], dtype=np.float64) for m in models]))
    seqs = [s for cs in class_seqs for s in cs]
    sym, offs = _pack(seqs)
    class_offs = np.zeros(len(class_seqs) + 1, dtype=np.int64)
    class_offs[1:] = np.cumsum([len(cs) for cs in class_seqs])
    cap = 4096
    hist, n = np.zeros((K, cap)), np.zeros(K, dtype=np.int32)
    check(lib.e2vq_hmm_train_classes(device, N, M, K, pi.ctypes.data, A.ctypes.data, B.ctypes.data, sym.ctypes.data,
                                     offs.ctypes.data, len(seqs), class_offs.ctypes.data, float(epsilon), float(val_auto),
                                     int(max_iterations), hist.ctypes.data, cap, n.ctypes.data))
    return [(pi[k].copy(), A[k].copy(), B[k].copy(), list(hist[k, :n[k]])) for k in range(K)]


def train_grid(models, seqs, ranges, epsilon=1e-5, val_auto=0.3, max_iterations=-1, device=0):
    """Baum-Welch of K models of any (N, M) in one batched training: models = [(pi, A, B)],
    seqs = [uint16 arrays] shared by all, ranges = [(lo, hi)] the sequences seqs[lo:hi] model k trains on (ranges may
    overlap) -> [(pi, A, B, [sum_log_prob per E-step])], each as `train` on its slice"""
    K = len(models)
    if K != len(ranges):
        raise ValueError(f"{K} models for {len(ranges)} sequence ranges")
    ms = [tuple(np.asarray(x, dtype=np.float64) for x in m) for m in models]
    Ns = np.array([len(m[0]) for m in ms], dtype=np.int32)
    Ms = np.array([m[2].shape[1] if m[2].ndim == 2 else 0 for m in ms], dtype=np.int32)
    sizes = [m[0].size + m[1].size + m[2].size for m in ms]
    param_offs = np.zeros(K, dtype=np.int64)
    param_offs[1:] = np.cumsum(sizes)[:-1]
    params = np.ascontiguousarray(np.concatenate([np.concatenate([x.ravel() for x in m]) for m in ms]))
    sym, offs = _pack(seqs)
    lo = np.array([r[0] for r in ranges], dtype=np.int64)
    hi = np.array([r[1] for r in ranges], dtype=np.int64)
    cap = 4096
    hist, n = np.zeros((K, cap)), np.zeros(K, dtype=np.int32)
    check(lib.e2vq_hmm_train_grid(device, K, Ns.ctypes.data, Ms.ctypes.data, params.ctypes.data, param_offs.ctypes.data,
                                  sym.ctypes.data, offs.ctypes.data, len(seqs), lo.ctypes.data, hi.ctypes.data,
                                  float(epsilon), float(val_auto), int(max_iterations), hist.ctypes.data, cap,
                                  n.ctypes.data))
    out = []
    for k, (N, M, o) in enumerate(zip(Ns, Ms, param_offs)):
        p = params[o:o + sizes[k]]
        out.append((p[:N].copy(), p[N:N + N * N].reshape(N, N).copy(), p[N + N * N:].reshape(N, M).copy(),
                    list(hist[k, :n[k]])))
    return out


def viterbi(pi, A, B, seqs, device=0, want_path=True):
    """most likely state sequences: dict(path=[uint16 arrays] or None, log_prob=(S,), status=(S,))"""
    pi, A, B = (np.ascontiguousarray(x, dtype=np.float64) for x in (pi, A, B))
    N, M, S = len(pi), B.shape[1], len(seqs)
    sym, offs = _pack(seqs)
    lp, st = np.zeros(S), np.zeros(S, dtype=np.int32)
    path = np.zeros(max(int(offs[-1]), 1), dtype=np.uint16) if want_path else None
    check(lib.e2vq_hmm_viterbi(device, N, M, pi.ctypes.data, A.ctypes.data, B.ctypes.data, sym.ctypes.data, offs.ctypes.data,
                               S, path.ctypes.data if want_path else None, lp.ctypes.data, st.ctypes.data))
    paths = [path[offs[s]:offs[s + 1]].copy() for s in range(S)] if want_path else None
    return dict(path=paths, log_prob=lp, status=st)


def scan_windows(offs, window, hop=None):
    """window offsets of `scan` (host only): stream s has (T_s - window) // hop + 1 windows when T_s >= window, else none"""
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    win_offs = np.zeros(len(offs), dtype=np.int64)
    check(lib.e2vq_hmm_scan_windows(offs.ctypes.data, len(offs) - 1, int(window), int(window if hop is None else hop),
                                    win_offs.ctypes.data))
    return win_offs


def scan(models, sym, offs, window, hop=None, device=0, matrix=True):
    """the models over sliding windows of whole symbol streams: models = [(pi, A, B)] sharing M; sym =
    the concatenated uint16 symbols of the streams -- a numpy array, or a device tensor (torch, dtype uint16 or int16, on
    `device`) as lpc.features takes frames --, offs = their S + 1 offsets; windows of `window` symbols every `hop` (default:
    window).  -> dict: win_offs (S + 1), best / second (W,) model indices with best_log_prob / second_log_prob, and with
    `matrix` the (W, K) arrays mant / exp2 / status / log_prob, each entry what `score` gives for that window's symbols"""
    K = len(models)
    ms = [tuple(np.ascontiguousarray(x, dtype=np.float64) for x in m) for m in models]
    Ns = (C.c_int * max(K, 1))(*[len(m[0]) for m in ms])
    ptr = lambda i: (C.c_void_p * max(K, 1))(*[m[i].ctypes.data for m in ms])
    M = ms[0][2].shape[1] if K else 0
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    S = len(offs) - 1
    hop = window if hop is None else hop
    on_device = hasattr(sym, "data_ptr")
    if on_device:
        if not sym.is_contiguous() or sym.element_size() != 2:
            raise ValueError("a device symbol tensor must be contiguous with 2-byte elements")
        sym_ptr = sym.data_ptr()
    else:
        sym = np.ascontiguousarray(sym, dtype=np.uint16)
        sym_ptr = sym.ctypes.data
    win_offs = np.zeros(S + 1, dtype=np.int64)
    if int(window) >= 1 and int(hop) >= 1 and K >= 1:
        win_offs = scan_windows(offs, window, hop)
    W = int(win_offs[-1])
    best, second = np.zeros(W, dtype=np.int32), np.zeros(W, dtype=np.int32)
    lp1, lp2 = np.zeros(W), np.zeros(W)
    out = dict(win_offs=win_offs, best=best, best_log_prob=lp1, second=second, second_log_prob=lp2)
    mat = [None] * 4
    if matrix:
        n = max(K, 0)
        out.update(mant=np.zeros((W, n)), exp2=np.zeros((W, n), dtype=np.int64), status=np.zeros((W, n), dtype=np.int32),
                   log_prob=np.zeros((W, n)))
        mat = [out[k].ctypes.data for k in ("mant", "exp2", "status", "log_prob")]
    check(lib.e2vq_hmm_scan(device, K, Ns, M, ptr(0), ptr(1), ptr(2), sym_ptr, offs.ctypes.data, S, int(window), int(hop),
                            win_offs.ctypes.data, *mat, best.ctypes.data, lp1.ctypes.data, second.ctypes.data,
                            lp2.ctypes.data, int(on_device)))
    return out


def scan_last_kernel_ms():
    return _kernel_ms(lib.e2vq_hmm_scan_last_kernel_ms)


def scan_files(model_filenames, input_filenames, window, hop=None, codebook=None, P=36, W_ms=45, O_ms=15, min_margin=0.0,
               csv=None):
    """`hmm scan`: every input (.wav, .prd or .seq) under the models over sliding windows; per input a
    block on stdout and, with `csv` (a directory, or a .csv file for one input), a CSV of the windows"""
    m, _k1 = _strs(model_filenames)
    f, _k2 = _strs(input_filenames)
    check(lib.e2vq_hmm_scan_files(m, len(model_filenames), str(codebook).encode() if codebook else None, f,
                                  len(input_filenames), int(P), int(W_ms), int(O_ms), int(window),
                                  int(window if hop is None else hop), float(min_margin), str(csv).encode() if csv else None))


def segments_of(cls, entered, gbest, log_prob, ln_switch):
    """the segments of one stream from its per-frame outputs (host arithmetic): a list of dicts begin, end
    (exclusive), cls, log_prob -- the segment [b, e) runs from one entered frame to the next"""
    T = len(cls)
    starts = [int(t) for t in np.flatnonzero(np.asarray(entered))]
    out = []
    for b, e in zip(starts, starts[1:] + [T]):
        hi = float(log_prob) if e == T else float(gbest[e])
        lo = 0.0 if b == 0 else float(gbest[b]) + float(ln_switch)
        with np.errstate(invalid="ignore"):
            out.append(dict(begin=b, end=e, cls=int(cls[b]), log_prob=float(np.float64(hi) - np.float64(lo))))
    return out


def segment(models, sym, offs, ln_switch, device=0):
    """the most likely path of whole symbol streams through the class loop of the models: models =
    [(pi, A, B)] sharing M, each of at most 64 states; sym, offs as `scan` takes them (numpy, or a device tensor);
    ln_switch <= 0: the log of the price of starting a segment (-inf: never).  -> dict: per frame cls / state (uint16),
    entered (uint8), gbest; per stream log_prob, status; and segments = per stream the list `segments_of` gives"""
    K = len(models)
    ms = [tuple(np.ascontiguousarray(x, dtype=np.float64) for x in m) for m in models]
    Ns = (C.c_int * max(K, 1))(*[len(m[0]) for m in ms])
    ptr = lambda i: (C.c_void_p * max(K, 1))(*[m[i].ctypes.data for m in ms])
    M = ms[0][2].shape[1] if K else 0
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    S = len(offs) - 1
    on_device = hasattr(sym, "data_ptr")
    if on_device:
        if not sym.is_contiguous() or sym.element_size() != 2:
            raise ValueError("a device symbol tensor must be contiguous with 2-byte elements")
        sym_ptr = sym.data_ptr()
    else:
        sym = np.ascontiguousarray(sym, dtype=np.uint16)
        sym_ptr = sym.ctypes.data
    n = max(int(offs[-1]), 1)
    cls, state = np.zeros(n, dtype=np.uint16), np.zeros(n, dtype=np.uint16)
    entered, gbest = np.zeros(n, dtype=np.uint8), np.zeros(n)
    lp, st = np.zeros(max(S, 1)), np.zeros(max(S, 1), dtype=np.int32)
    check(lib.e2vq_hmm_segment(device, K, Ns, M, ptr(0), ptr(1), ptr(2), sym_ptr, offs.ctypes.data, S, float(ln_switch),
                               cls.ctypes.data, state.ctypes.data, entered.ctypes.data, gbest.ctypes.data, lp.ctypes.data,
                               st.ctypes.data, int(on_device)))
    T = int(offs[-1])
    out = dict(cls=cls[:T], state=state[:T], entered=entered[:T], gbest=gbest[:T], log_prob=lp[:S], status=st[:S])
    out["segments"] = [segments_of(out["cls"][a:b], out["entered"][a:b], out["gbest"][a:b], lp[s], ln_switch)
                       for s, (a, b) in enumerate(zip(offs[:-1], offs[1:]))]
    return out


def segment_last_kernel_ms():
    return _kernel_ms(lib.e2vq_hmm_segment_last_kernel_ms)


class SegmentStream:
    """`segment` on one stream that arrives piece by piece: a context manager around a decoder session.
    models, ln_switch as `segment` takes them.  `feed(sym)` (numpy, or a device tensor), `flush()` (the buffered remainder
    is processed) and `close()` each return a dict of the frames that became final with the call: first (the absolute
    frame of the first), cls, state, entered, gbest, and segments -- the segments completed since the last call, as
    `segments_of` gives them with absolute frames: [b, e) is complete once frame e is final and entered, or at close.
    After `close`, log_prob and status are set.  The block length and the pending budget are read from
    ECOZ2_HMM_SEGMENT_STREAM_BLOCK and ECOZ2_HMM_SEGMENT_STREAM_PENDING_BYTES when the session is opened, and
    ECOZ2_HMM_SEGMENT_BODY is honoured as by `segment`."""

    def __init__(self, models, ln_switch, device=0):
        K = len(models)
        ms = [tuple(np.ascontiguousarray(x, dtype=np.float64) for x in m) for m in models]
        Ns = (C.c_int * max(K, 1))(*[len(m[0]) for m in ms])
        ptr = lambda i: (C.c_void_p * max(K, 1))(*[m[i].ctypes.data for m in ms])
        M = ms[0][2].shape[1] if K else 0
        self._h = C.c_void_p()
        self.ln_switch = float(ln_switch)
        self.final_frames_ = 0
        self.log_prob = None
        self.status = None
        self._open = None  # the segment that is not complete yet: (begin, cls, lo)
        check(lib.e2vq_hmm_segment_stream_open(device, K, Ns, M, ptr(0), ptr(1), ptr(2), self.ln_switch, C.byref(self._h)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def free(self):
        if self._h:
            lib.e2vq_hmm_segment_stream_free(self._h)
            self._h = C.c_void_p()

    __del__ = free

    @property
    def final_frames(self):
        """frames final so far"""
        return self.final_frames_

    def _take(self, end_log_prob=None):
        n = max(self.final_frames_, 1)
        cls, state = np.zeros(n, dtype=np.uint16), np.zeros(n, dtype=np.uint16)
        entered, gbest = np.zeros(n, dtype=np.uint8), np.zeros(n)
        first, count = C.c_int64(), C.c_int64()
        check(lib.e2vq_hmm_segment_stream_take(self._h, n, cls.ctypes.data, state.ctypes.data, entered.ctypes.data, gbest.ctypes.data,
                                               C.byref(first), C.byref(count)))
        c, f0 = count.value, first.value
        out = dict(first=f0, cls=cls[:c], state=state[:c], entered=entered[:c], gbest=gbest[:c], segments=[])

        def complete(end, hi):
            b, k, lo = self._open
            with np.errstate(invalid="ignore"):
                out["segments"].append(dict(begin=b, end=end, cls=k, log_prob=float(np.float64(hi) - np.float64(lo))))

        for i in np.flatnonzero(out["entered"]):
            t = f0 + int(i)
            if self._open is not None:
                complete(t, float(gbest[i]))
            self._open = (t, int(cls[i]), 0.0 if t == 0 else float(gbest[i]) + self.ln_switch)
        if end_log_prob is not None and self._open is not None:
            complete(f0 + c, end_log_prob)
            self._open = None
        return out

    def feed(self, sym):
        on_device = hasattr(sym, "data_ptr")
        if on_device:
            if not sym.is_contiguous() or sym.element_size() != 2:
                raise ValueError("a device symbol tensor must be contiguous with 2-byte elements")
            sym_ptr, n = sym.data_ptr(), sym.numel()
        else:
            sym = np.ascontiguousarray(sym, dtype=np.uint16)
            sym_ptr, n = sym.ctypes.data, sym.size
        fin = C.c_int64()
        rc = lib.e2vq_hmm_segment_stream_feed(self._h, sym_ptr, n, int(on_device), C.byref(fin))
        self.final_frames_ = max(self.final_frames_, fin.value)  # (a feed that fails may have processed blocks before it did)
        check(rc)
        return self._take()

    def flush(self):
        fin = C.c_int64()
        check(lib.e2vq_hmm_segment_stream_flush(self._h, C.byref(fin)))
        self.final_frames_ = fin.value
        return self._take()

    def close(self):
        lp, st, fin = C.c_double(), C.c_int(), C.c_int64()
        check(lib.e2vq_hmm_segment_stream_close(self._h, C.byref(lp), C.byref(st), C.byref(fin)))
        self.final_frames_, self.log_prob, self.status = fin.value, lp.value, st.value
        return self._take(end_log_prob=lp.value if st.value != 2 else None)

    def take(self):
        """the frames that are final and were not handed out yet (after a feed that failed, for instance)"""
        return self._take()

    def kernel_ms(self):
        ms = C.c_float()
        check(lib.e2vq_hmm_segment_stream_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def stats(self):
        """dict peak_pending (frames), device_bytes, commit_ms (coalescence and backtrack, part of kernel_ms)"""
        pk, by, ms = C.c_int64(), C.c_int64(), C.c_float()
        check(lib.e2vq_hmm_segment_stream_stats(self._h, C.byref(pk), C.byref(by), C.byref(ms)))
        return dict(peak_pending=pk.value, device_bytes=by.value, commit_ms=ms.value)


def segment_posteriors(models, sym, offs, ln_switch, device=0, body=None):
    """P(class at frame t | the whole stream) under the class loop `segment` decodes: arguments as
    `segment` takes them (sym a numpy array or a device tensor); the classes must pack into at most 16 wave-slots unless
    the looped body is chosen.  body: "auto", "resident" or "looped" (ECOZ2_HMM_POSTERIOR_BODY for this call: the looped
    body takes any number of wave-slots, "auto" uses it above 16; the same bits either way); None: what the environment says.
    -> dict: post (sum T_s, K), row offs[s] + t; per stream log_prob = ln P(O | loop) and status (0 ok, 1 the loop cannot
    emit the stream, 2 a symbol >= M; then the stream's rows are 0.0 and log_prob is -inf)"""
    K = len(models)
    ms = [tuple(np.ascontiguousarray(x, dtype=np.float64) for x in m) for m in models]
    Ns = (C.c_int * max(K, 1))(*[len(m[0]) for m in ms])
    ptr = lambda i: (C.c_void_p * max(K, 1))(*[m[i].ctypes.data for m in ms])
    M = ms[0][2].shape[1] if K else 0
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    S = len(offs) - 1
    on_device = hasattr(sym, "data_ptr")
    if on_device:
        if not sym.is_contiguous() or sym.element_size() != 2:
            raise ValueError("a device symbol tensor must be contiguous with 2-byte elements")
        sym_ptr = sym.data_ptr()
    else:
        sym = np.ascontiguousarray(sym, dtype=np.uint16)
        sym_ptr = sym.ctypes.data
    T = int(offs[-1])
    post = np.zeros((max(T, 1), max(K, 1)))
    lp, st = np.zeros(max(S, 1)), np.zeros(max(S, 1), dtype=np.int32)
    with _body_env("ECOZ2_HMM_POSTERIOR_BODY", body):
        check(lib.e2vq_hmm_segment_posteriors(device, K, Ns, M, ptr(0), ptr(1), ptr(2), sym_ptr, offs.ctypes.data, S, float(ln_switch),
                                              post.ctypes.data, lp.ctypes.data, st.ctypes.data, int(on_device)))
    return dict(post=post[:T], log_prob=lp[:S], status=st[:S])


def segment_posteriors_last_kernel_ms():
    return _kernel_ms(lib.e2vq_hmm_segment_posteriors_last_kernel_ms)


class PosteriorStream:
    """`segment_posteriors` on one stream that arrives piece by piece: a context manager around a posterior
    session.  models, ln_switch and body as `segment_posteriors` takes them (body: ECOZ2_HMM_POSTERIOR_BODY while the session
    opens, which fixes its body).  block B >= 1 and lookahead L >= 0, in frames: the rows of block b = the frames
    [b B, (b + 1) B) are ready once (b + 1) B + L symbols were fed, and are P(class at t | those symbols) -- the bits of
    `segment_posteriors` on that prefix; `close()` delivers the rest, conditioned on the whole stream.  `feed(sym)` (numpy, or
    a device tensor), `close()` and `take()` return (first, post): the absolute frame of the first row that became ready with
    the call, and the rows (count, K).  After `close`, log_prob and status are set (a stream of status 1 or 2: the rows that
    were not delivered before the event come as 0.0 with close, log_prob is -inf; the feed or close that meets a symbol >= M
    raises, and `take()` then hands out what is ready)."""

    def __init__(self, models, ln_switch, block=4096, lookahead=4096, device=0, body=None):
        self._h = C.c_void_p()  # (first: free, which __del__ calls, reads it whatever fails below)
        K = len(models)
        ms = [tuple(np.ascontiguousarray(x, dtype=np.float64) for x in m) for m in models]
        Ns = (C.c_int * max(K, 1))(*[len(m[0]) for m in ms])
        ptr = lambda i: (C.c_void_p * max(K, 1))(*[m[i].ctypes.data for m in ms])
        M = ms[0][2].shape[1] if K else 0
        self.K = K
        self.ready_frames_ = 0
        self._taken = 0  # rows handed out so far
        self.log_prob = None
        self.status = None
        with _body_env("ECOZ2_HMM_POSTERIOR_BODY", body):
            check(lib.e2vq_hmm_posterior_stream_open(device, K, Ns, M, ptr(0), ptr(1), ptr(2), float(ln_switch), int(block),
                                                     int(lookahead), C.byref(self._h)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def free(self):
        if self._h:
            lib.e2vq_hmm_posterior_stream_free(self._h)
            self._h = C.c_void_p()

    __del__ = free

    @property
    def ready_frames(self):
        """frames delivered so far"""
        return self.ready_frames_

    def take(self):
        """(first, post): the rows that are ready and were not handed out yet"""
        n = max(self.ready_frames_ - self._taken, 0)  # (what waits in the session, not the stream so far)
        post = np.zeros((max(n, 1), max(self.K, 1)))
        first, count = C.c_int64(), C.c_int64()
        check(lib.e2vq_hmm_posterior_stream_take(self._h, n, post.ctypes.data, C.byref(first), C.byref(count)))
        self._taken = first.value + count.value
        return first.value, post[:count.value]

    def feed(self, sym):
        on_device = hasattr(sym, "data_ptr")
        if on_device:
            if not sym.is_contiguous() or sym.element_size() != 2:
                raise ValueError("a device symbol tensor must be contiguous with 2-byte elements")
            sym_ptr, n = sym.data_ptr(), sym.numel()
        else:
            sym = np.ascontiguousarray(sym, dtype=np.uint16)
            sym_ptr, n = sym.ctypes.data, sym.size
        ready = C.c_int64()
        rc = lib.e2vq_hmm_posterior_stream_feed(self._h, sym_ptr, n, int(on_device), C.byref(ready))
        self.ready_frames_ = max(self.ready_frames_, ready.value)  # (a feed that fails may have delivered blocks before it did)
        check(rc)
        return self.take()

    def close(self):
        lp, st, ready = C.c_double(), C.c_int(-1), C.c_int64(-1)
        rc = lib.e2vq_hmm_posterior_stream_close(self._h, C.byref(lp), C.byref(st), C.byref(ready))
        if ready.value >= 0:  # (a close that meets a symbol >= M fails after it has set its outputs)
            self.ready_frames_, self.log_prob, self.status = ready.value, lp.value, st.value
        check(rc)
        return self.take()

    def kernel_ms(self):
        ms = C.c_float()
        check(lib.e2vq_hmm_posterior_stream_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def stats(self):
        """dict device_bytes, ring_rows, launches, backward_frames (the frames the backward passes walked)"""
        by, rows, ln, bw = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        check(lib.e2vq_hmm_posterior_stream_stats(self._h, C.byref(by), C.byref(rows), C.byref(ln), C.byref(bw)))
        return dict(device_bytes=by.value, ring_rows=rows.value, launches=ln.value, backward_frames=bw.value)


def segments_of_trans(cls, entered, exit_score, log_prob, ln_trans):
    """`segments_of` under the K x K prices ln_trans: the segment that starts at b > 0 paid
    ln_trans[cls[b - 1]][cls[b]]"""
    lt = np.asarray(ln_trans, dtype=np.float64)
    T = len(cls)
    starts = [int(t) for t in np.flatnonzero(np.asarray(entered))]
    out = []
    for b, e in zip(starts, starts[1:] + [T]):
        hi = np.float64(log_prob if e == T else exit_score[e])
        with np.errstate(invalid="ignore"):
            lo = np.float64(0.0) if b == 0 else np.float64(exit_score[b]) + lt[int(cls[b - 1]), int(cls[b])]
            out.append(dict(begin=b, end=e, cls=int(cls[b]), log_prob=float(hi - lo)))
    return out


def segment_trans(models, sym, offs, ln_trans, device=0, body=None):
    """`segment` under a K x K matrix of class-to-class prices: ln_trans[f][k] <= 0 (or -inf) is the log of
    the price of leaving class f and entering class k; the classes must pack into at most 16 wave-slots unless the looped body
    is chosen.  body: "auto", "resident" or "looped" (ECOZ2_HMM_SEGMENT_TRANS_BODY for this call: the looped body takes any
    number of slots, auto picks it above 16; the path is the same bit for bit); None leaves the environment alone.  -> the
    dict of `segment` with exit_score in the place of gbest: exit_score[t] = the best score in the class of frame t - 1 at
    t - 1"""
    K = len(models)
    ms = [tuple(np.ascontiguousarray(x, dtype=np.float64) for x in m) for m in models]
    Ns = (C.c_int * max(K, 1))(*[len(m[0]) for m in ms])
    ptr = lambda i: (C.c_void_p * max(K, 1))(*[m[i].ctypes.data for m in ms])
    M = ms[0][2].shape[1] if K else 0
    lt = np.ascontiguousarray(ln_trans, dtype=np.float64)
    if lt.shape != (K, K):
        raise ValueError(f"ln_trans has the shape {lt.shape}, not ({K}, {K})")
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    S = len(offs) - 1
    on_device = hasattr(sym, "data_ptr")
    if on_device:
        if not sym.is_contiguous() or sym.element_size() != 2:
            raise ValueError("a device symbol tensor must be contiguous with 2-byte elements")
        sym_ptr = sym.data_ptr()
    else:
        sym = np.ascontiguousarray(sym, dtype=np.uint16)
        sym_ptr = sym.ctypes.data
    n = max(int(offs[-1]), 1)
    cls, state = np.zeros(n, dtype=np.uint16), np.zeros(n, dtype=np.uint16)
    entered, ex = np.zeros(n, dtype=np.uint8), np.zeros(n)
    lp, st = np.zeros(max(S, 1)), np.zeros(max(S, 1), dtype=np.int32)
    with _body_env("ECOZ2_HMM_SEGMENT_TRANS_BODY", body):
        check(lib.e2vq_hmm_segment_trans(device, K, Ns, M, ptr(0), ptr(1), ptr(2), sym_ptr, offs.ctypes.data, S, lt.ctypes.data,
                                         cls.ctypes.data, state.ctypes.data, entered.ctypes.data, ex.ctypes.data, lp.ctypes.data,
                                         st.ctypes.data, int(on_device)))
    T = int(offs[-1])
    out = dict(cls=cls[:T], state=state[:T], entered=entered[:T], exit_score=ex[:T], log_prob=lp[:S], status=st[:S])
    out["segments"] = [segments_of_trans(out["cls"][a:b], out["entered"][a:b], out["exit_score"][a:b], lp[s], lt)
                       for s, (a, b) in enumerate(zip(offs[:-1], offs[1:]))]
    return out


def segment_trans_last_kernel_ms():
    return _kernel_ms(lib.e2vq_hmm_segment_trans_last_kernel_ms)


class SegmentTransStream(SegmentStream):
    """`segment_trans` on one stream that arrives piece by piece: `SegmentStream` under the K x K prices
    ln_trans of `segment_trans` (the classes must pack into at most 16 wave-slots unless body -- "auto", "resident" or
    "looped", ECOZ2_HMM_SEGMENT_TRANS_BODY while the session opens, which fixes its body -- chooses the looped one).  feed /
    flush / close / take return the
    dict of `SegmentStream` with exit_score in the place of gbest; segments follow `segments_of_trans` with absolute frames
    (the class of the last final frame is kept across calls: the segment that starts at b paid
    ln_trans[cls[b - 1]][cls[b]])."""

    def __init__(self, models, ln_trans, device=0, body=None):
        K = len(models)
        ms = [tuple(np.ascontiguousarray(x, dtype=np.float64) for x in m) for m in models]
        Ns = (C.c_int * max(K, 1))(*[len(m[0]) for m in ms])
        ptr = lambda i: (C.c_void_p * max(K, 1))(*[m[i].ctypes.data for m in ms])
        M = ms[0][2].shape[1] if K else 0
        lt = np.ascontiguousarray(ln_trans, dtype=np.float64)
        self._h = C.c_void_p()
        if lt.shape != (K, K):
            raise ValueError(f"ln_trans has the shape {lt.shape}, not ({K}, {K})")
        self.ln_trans = lt
        self.final_frames_ = 0
        self.log_prob = None
        self.status = None
        self._open = None  # the segment that is not complete yet: (begin, cls, lo)
        self._last_cls = None  # the class of the last frame handed out
        with _body_env("ECOZ2_HMM_SEGMENT_TRANS_BODY", body):
            check(lib.e2vq_hmm_segment_trans_stream_open(device, K, Ns, M, ptr(0), ptr(1), ptr(2), lt.ctypes.data, C.byref(self._h)))

    def _take(self, end_log_prob=None):
        n = max(self.final_frames_, 1)
        cls, state = np.zeros(n, dtype=np.uint16), np.zeros(n, dtype=np.uint16)
        entered, ex = np.zeros(n, dtype=np.uint8), np.zeros(n)
        first, count = C.c_int64(), C.c_int64()
        check(lib.e2vq_hmm_segment_stream_take(self._h, n, cls.ctypes.data, state.ctypes.data, entered.ctypes.data, ex.ctypes.data,
                                               C.byref(first), C.byref(count)))
        c, f0 = count.value, first.value
        out = dict(first=f0, cls=cls[:c], state=state[:c], entered=entered[:c], exit_score=ex[:c], segments=[])

        def complete(end, hi):
            b, k, lo = self._open
            with np.errstate(invalid="ignore"):
                out["segments"].append(dict(begin=b, end=end, cls=k, log_prob=float(np.float64(hi) - np.float64(lo))))

        for i in np.flatnonzero(out["entered"]):
            t = f0 + int(i)
            if self._open is not None:
                complete(t, float(ex[i]))
            lo = np.float64(0.0)
            if t > 0:
                before = int(cls[i - 1]) if i > 0 else self._last_cls
                with np.errstate(invalid="ignore"):
                    lo = np.float64(ex[i]) + self.ln_trans[before, int(cls[i])]
            self._open = (t, int(cls[i]), lo)
        if c > 0:
            self._last_cls = int(cls[c - 1])
        if end_log_prob is not None and self._open is not None:
            complete(f0 + c, end_log_prob)
            self._open = None
        return out


def segment_trans_posteriors(models, sym, offs, ln_trans, device=0):
    """`segment_posteriors` under the K x K prices of `segment_trans`: P(class at frame t | the whole
    stream) under the loop `segment_trans` decodes; ln_trans[f][k] <= 0 (or -inf) as there; the classes must pack into at
    most 16 wave-slots unless the looped body is chosen (ECOZ2_HMM_TRANS_FB_BODY; `trans_fb_body` sets it for a call: the looped
    body takes any number of slots, auto picks it above 16, the posteriors are the same bit for bit).  sym: a numpy array or a
    device tensor.  -> the dict of
    `segment_posteriors`: post (sum T_s, K), per stream log_prob and status"""
    K = len(models)
    ms = [tuple(np.ascontiguousarray(x, dtype=np.float64) for x in m) for m in models]
    Ns = (C.c_int * max(K, 1))(*[len(m[0]) for m in ms])
    ptr = lambda i: (C.c_void_p * max(K, 1))(*[m[i].ctypes.data for m in ms])
    M = ms[0][2].shape[1] if K else 0
    lt = np.ascontiguousarray(ln_trans, dtype=np.float64)
    if lt.shape != (K, K):
        raise ValueError(f"ln_trans has the shape {lt.shape}, not ({K}, {K})")
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    S = len(offs) - 1
    on_device = hasattr(sym, "data_ptr")
    if on_device:
        if not sym.is_contiguous() or sym.element_size() != 2:
            raise ValueError("a device symbol tensor must be contiguous with 2-byte elements")
        sym_ptr = sym.data_ptr()
    else:
        sym = np.ascontiguousarray(sym, dtype=np.uint16)
        sym_ptr = sym.ctypes.data
    T = int(offs[-1])
    post = np.zeros((max(T, 1), max(K, 1)))
    lp, st = np.zeros(max(S, 1)), np.zeros(max(S, 1), dtype=np.int32)
    check(lib.e2vq_hmm_segment_trans_posteriors(device, K, Ns, M, ptr(0), ptr(1), ptr(2), sym_ptr, offs.ctypes.data, S, lt.ctypes.data,
                                                post.ctypes.data, lp.ctypes.data, st.ctypes.data, int(on_device)))
    return dict(post=post[:T], log_prob=lp[:S], status=st[:S])


def segment_trans_posteriors_last_kernel_ms():
    return _kernel_ms(lib.e2vq_hmm_segment_trans_posteriors_last_kernel_ms)


def class_transitions(label_sequences, K, alpha=1.0):
    """the K x K prices of `segment_trans` from sequences of class labels in [0, K) (host only): bigrams
    are counted within each sequence; ln((c[f][k] + alpha) / (sum_k' c[f][k'] + alpha K)), -inf for an unseen pair at alpha = 0"""
    arrs = [np.ascontiguousarray(s, dtype=np.int32) for s in label_sequences]
    offs = np.zeros(len(arrs) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(a) for a in arrs])
    labels = np.ascontiguousarray(np.concatenate(arrs)) if arrs and offs[-1] else np.zeros(1, dtype=np.int32)
    lt = np.zeros((max(int(K), 1), max(int(K), 1)))
    check(lib.e2vq_hmm_class_transitions(labels.ctypes.data, offs.ctypes.data, len(arrs), int(K), float(alpha), lt.ctypes.data))
    return lt


def read_class_transitions(path, class_names):
    """the matrix of a transitions file in the order of class_names (the models' classes)"""
    names, _k = _strs(class_names)
    lt = np.zeros((max(len(class_names), 1),) * 2)
    check(lib.e2vq_hmm_transitions_read(str(path).encode(), len(class_names), names, lt.ctypes.data))
    return lt


def write_class_transitions(path, class_names, ln_trans):
    """the transitions file `hmm segment --class-transitions` reads: header class,<names>, a row per class"""
    names, _k = _strs(class_names)
    lt = np.ascontiguousarray(ln_trans, dtype=np.float64)
    if lt.shape != (len(class_names),) * 2:
        raise ValueError(f"ln_trans has the shape {lt.shape} for {len(class_names)} classes")
    check(lib.e2vq_hmm_transitions_write(str(path).encode(), len(class_names), names, lt.ctypes.data))


def class_transitions_files(model_filenames, input_filenames, out_csv, alpha=1.0):
    """`hmm transitions`: the transitions file of the models' classes from segment CSVs or selection tables"""
    m, _k1 = _strs(model_filenames)
    f, _k2 = _strs(input_filenames)
    check(lib.e2vq_hmm_transitions_files(m, len(model_filenames), f, len(input_filenames), float(alpha), str(out_csv).encode()))


def _trans_args(models, sym, offs, ln_trans):
    """the arguments `transitions_estep` and `train_transitions` share -> (the C arguments up to S, a copy of ln_trans (K, K),
    on_device, S, what must stay alive)"""
    K = len(models)
    ms = [tuple(np.ascontiguousarray(x, dtype=np.float64) for x in m) for m in models]
    Ns = (C.c_int * max(K, 1))(*[len(m[0]) for m in ms])
    ptrs = [(C.c_void_p * max(K, 1))(*[m[i].ctypes.data for m in ms]) for i in range(3)]
    M = ms[0][2].shape[1] if K else 0
    lt = np.array(ln_trans, dtype=np.float64, order="C")
    if lt.shape != (K, K):
        raise ValueError(f"ln_trans has the shape {lt.shape}, not ({K}, {K})")
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    on_device = hasattr(sym, "data_ptr")
    if on_device:
        if not sym.is_contiguous() or sym.element_size() != 2:
            raise ValueError("a device symbol tensor must be contiguous with 2-byte elements")
        sym_ptr = sym.data_ptr()
    else:
        sym = np.ascontiguousarray(sym, dtype=np.uint16)
        sym_ptr = sym.ctypes.data
    S = len(offs) - 1
    return (K, Ns, M, *ptrs, sym_ptr, offs.ctypes.data, S), lt, int(on_device), S, (ms, sym, offs)


def transitions_acc_words(K):
    return int(lib.e2vq_hmm_transitions_acc_words(int(K)))


def transitions_estep(models, sym, offs, ln_trans, acc=None, device=0, body=None):
    """one E-step of Baum-Welch for the class-to-class prices: models, sym (a numpy array or a device tensor),
    offs and ln_trans as `segment_trans_posteriors` takes them -> dict acc (int64, 2 K^2 + 2: the limb pairs of the expected
    counts C[f][k], then the streams used and skipped; added to `acc` where one is given), per stream log_prob and status.
    body: "auto", "resident" or "looped" (ECOZ2_HMM_TRANS_FB_BODY for this call, as `trans_fb_body` sets it: resident takes at
    most 16 wave-slots of classes, looped any number, auto the looped one above 16; the same counts bit for bit); None leaves
    the environment alone"""
    c_args, lt, on_device, S, _keep = _trans_args(models, sym, offs, ln_trans)
    words = transitions_acc_words(len(models))
    if acc is None:
        acc = np.zeros(max(words, 2), dtype=np.int64)
    elif not (isinstance(acc, np.ndarray) and acc.dtype == np.int64 and acc.flags.c_contiguous and acc.size == words):
        raise ValueError(f"acc must be a contiguous int64 array of {words} words")
    lp, st = np.zeros(max(S, 1)), np.zeros(max(S, 1), dtype=np.int32)
    with trans_fb_body(body):
        check(lib.e2vq_hmm_transitions_estep(device, *c_args, lt.ctypes.data, acc.ctypes.data, lp.ctypes.data, st.ctypes.data, on_device))
    return dict(acc=acc, log_prob=lp[:S], status=st[:S])


def transitions_estep_last_kernel_ms():
    return _kernel_ms(lib.e2vq_hmm_transitions_estep_last_kernel_ms)


def train_transitions(models, sym, offs, ln_p=None, ln_switch=0.0, alpha=1.0, val_auto=0.3, max_iterations=-1, callback=None, device=0,
                      body=None):
    """Baum-Welch for the class-to-class prices to its stop: ln_p is the matrix as a transitions file holds it
    (None: every entry log(1 / K)), the effective price of an E-step ln_p + ln_switch -> (the trained ln_p (K, K), the sum of
    ln P per E-step); callback(var: str, val: float) per E-step; body as `transitions_estep` takes it (read once, before the first
    E-step)"""
    K = len(models)
    if ln_p is None:
        ln_p = np.full((K, K), math.log(1.0 / K)) if K else np.zeros((0, 0))
    c_args, lt, on_device, _S, _keep = _trans_args(models, sym, offs, ln_p)
    cap = 1000
    hist = np.zeros(cap)
    n = C.c_int(0)
    cb = HMM_LEARN_CALLBACK((lambda v, x: callback(v.decode(), x)) if callback else (lambda _v, _x: None))
    with trans_fb_body(body):
        check(lib.e2vq_hmm_train_transitions(device, *c_args, lt.ctypes.data, float(ln_switch), float(alpha), float(val_auto),
                                             int(max_iterations), hist.ctypes.data, cap, C.byref(n), cb, on_device))
    return lt, hist[:n.value].copy()


def learn_transitions_files(model_filenames, input_filenames, out_csv, ln_switch, init=None, alpha=1.0, val_auto=0.3, max_iterations=-1,
                            codebook=None, P=36, W_ms=45, O_ms=15, body=None):
    """`hmm transitions --em`: the transitions file of the models' classes by Baum-Welch from the inputs (.wav,
    .prd or .seq), from the file `init` or the uniform matrix; writes out_csv and <out_csv>.em.csv; body as `transitions_estep` takes it"""
    m, _k1 = _strs(model_filenames)
    f, _k2 = _strs(input_filenames)
    with trans_fb_body(body):
        check(lib.e2vq_hmm_learn_transitions_files(m, len(model_filenames), str(codebook).encode() if codebook else None, f,
                                                   len(input_filenames), int(P), int(W_ms), int(O_ms), float(ln_switch),
                                                   str(init).encode() if init else None, float(alpha), float(val_auto),
                                                   int(max_iterations), str(out_csv).encode()))


def loop_estep(models, sym, offs, ln_trans, acc_trans=None, device=0):
    """one E-step of Baum-Welch for the class models under the class loop: models, sym (a numpy array or a
    device tensor), offs and ln_trans as `transitions_estep` takes them -> dict acc (per class its int64 accumulator words, the
    layout of `acc_words`), per stream log_prob and status.  acc_trans: None, True (a new table) or an int64 array of
    `transitions_acc_words(K)` words to add into -> also acc_trans, the grammar counts of `transitions_estep`"""
    c_args, lt, on_device, S, keep = _trans_args(models, sym, offs, ln_trans)
    ms, M = keep[0], c_args[2]
    acc = [np.zeros(int(lib.e2vq_hmm_acc_words(len(m[0]), M)), dtype=np.int64) for m in ms]
    accp = (C.c_void_p * max(len(acc), 1))(*[x.ctypes.data for x in acc])
    words = transitions_acc_words(len(models))
    if acc_trans is True:
        acc_trans = np.zeros(max(words, 2), dtype=np.int64)
    elif acc_trans is not None and not (isinstance(acc_trans, np.ndarray) and acc_trans.dtype == np.int64 and
                                        acc_trans.flags.c_contiguous and acc_trans.size == words):
        raise ValueError(f"acc_trans must be a contiguous int64 array of {words} words")
    lp, st = np.zeros(max(S, 1)), np.zeros(max(S, 1), dtype=np.int32)
    check(lib.e2vq_hmm_loop_estep(device, *c_args, lt.ctypes.data, accp, acc_trans.ctypes.data if acc_trans is not None else None,
                                  lp.ctypes.data, st.ctypes.data, on_device))
    out = dict(acc=acc, log_prob=lp[:S], status=st[:S])
    if acc_trans is not None:
        out["acc_trans"] = acc_trans
    return out


def loop_estep_last_kernel_ms():
    return _kernel_ms(lib.e2vq_hmm_loop_estep_last_kernel_ms)


def train_loop(models, sym, offs, ln_p=None, ln_switch=0.0, train_transitions=False, frozen=None, alpha=1.0, epsilon=1e-5, val_auto=0.3,
               max_iterations=-1, callback=None, device=0):
    """Baum-Welch for the class models under the class loop to its stop: ln_p is the matrix as a transitions
    file holds it (None: zeros), the effective price of an E-step ln_p + ln_switch; train_transitions: the matrix is
    re-estimated with the models (alpha as `train_transitions` takes it); frozen: per class a flag, a class whose flag is set
    keeps its model -> (the trained models [(pi, A, B)], ln_p (K, K), the sum of ln P per E-step); callback(var: str,
    val: float) per E-step"""
    K = len(models)
    if ln_p is None:
        ln_p = np.zeros((K, K))
    models = [tuple(np.array(x, dtype=np.float64, order="C") for x in m) for m in models]  # (copies: the call writes them)
    c_args, lt, on_device, _S, _keep = _trans_args(models, sym, offs, ln_p)
    fz = None
    if frozen is not None:
        fz = np.ascontiguousarray(np.asarray(frozen) != 0, dtype=np.uint8)
        if fz.shape != (K,):
            raise ValueError(f"frozen has the shape {fz.shape}, not ({K},)")
    cap = 1000
    hist = np.zeros(cap)
    n = C.c_int(0)
    cb = HMM_LEARN_CALLBACK((lambda v, x: callback(v.decode(), x)) if callback else (lambda _v, _x: None))
    check(lib.e2vq_hmm_train_loop(device, *c_args, lt.ctypes.data, float(ln_switch), int(bool(train_transitions)),
                                  fz.ctypes.data if fz is not None else None, float(alpha), float(epsilon), float(val_auto),
                                  int(max_iterations), hist.ctypes.data, cap, C.byref(n), cb, on_device))
    return _keep[0], lt, hist[:n.value].copy()


def learn_loop_files(model_filenames, input_filenames, out_dir, ln_switch, class_transitions=None, train_transitions=False, freeze=(),
                     alpha=1.0, hmm_epsilon=1e-5, val_auto=0.3, max_iterations=-1, codebook=None, P=36, W_ms=45, O_ms=15, callback=None):
    """`hmm learn --loop`: the models of the files re-estimated from the inputs (.wav, .prd or .seq) under the
    class loop, from the transitions file class_transitions or a matrix of zeros; freeze: class names whose models stay; writes
    <out_dir>/<class>.hmm for every class, <out_dir>/loop.csv and, with train_transitions, <out_dir>/transitions.csv"""
    m, _k1 = _strs(model_filenames)
    f, _k2 = _strs(input_filenames)
    z, _k3 = _strs(list(freeze))
    cb = HMM_LEARN_CALLBACK((lambda v, x: callback(v.decode(), x)) if callback else (lambda _v, _x: None))
    check(lib.e2vq_hmm_learn_loop_files(m, len(model_filenames), str(codebook).encode() if codebook else None, f, len(input_filenames),
                                        int(P), int(W_ms), int(O_ms), float(ln_switch),
                                        str(class_transitions).encode() if class_transitions else None, int(bool(train_transitions)),
                                        z, len(freeze), float(alpha), float(hmm_epsilon), float(val_auto), int(max_iterations),
                                        str(out_dir).encode(), cb))


def segment_files(model_filenames, input_filenames, ln_switch, codebook=None, P=36, W_ms=45, O_ms=15, csv=None, posteriors=False,
                  frame_posteriors=None, class_transitions=None, continuous=None, body=None, grammar_posteriors=False,
                  grammar_continuous=None, grammar_body=None, grammar_posteriors_body=None, continuous_posteriors=None, block=4096,
                  lookahead=4096):
    """`hmm segment`: every input (.wav, .prd or .seq) decoded once under the models; per input a block on
    stdout and, with `csv` (a directory, or a .csv file for one input), a CSV of the segments.  posteriors (4.8.7): each
    segment's mean and least class posterior in the block and the CSV, and with frame_posteriors (a directory) a per-frame
    table for every input; body as `segment_posteriors` takes it.  class_transitions (4.8.8): a transitions file whose prices are added to ln_switch;
    grammar_posteriors (4.8.13): with class_transitions, the posteriors under those prices, reported as posteriors reports
    them (frame_posteriors is then taken too); grammar_posteriors_body ("auto", "resident" or "looped", as `transitions_estep`
    takes body) chooses their kernel body, and the decode of the same input follows it; it needs grammar_posteriors.  continuous
    (4.8.9): the name of the one recording whose consecutive pieces the inputs are -- one block, and with `csv` (a directory
    or a .csv file) one CSV, <csv>/<name>.csv.  grammar_continuous (4.8.15): with class_transitions, the same under the
    file's prices; it excludes continuous, the posteriors, frame_posteriors and body.  grammar_body ("auto", "resident" or
    "looped", as `segment_trans` takes body): the kernel body of the decoder under class_transitions, with or without
    grammar_continuous; it needs class_transitions and excludes grammar_posteriors, whose one choice is
    grammar_posteriors_body.  continuous_posteriors (4.8.17): the name of the one recording whose consecutive pieces the inputs
    are, decoded as by continuous and reported as by posteriors (one block, one CSV, and with frame_posteriors
    <frame_posteriors>/<name>.csv), the posteriors of a block of `block` frames conditioned on the recording up to `lookahead`
    frames behind it; it takes body and frame_posteriors and excludes every other mode"""
    m, _k1 = _strs(model_filenames)
    f, _k2 = _strs(input_filenames)
    if continuous_posteriors is not None:
        if (continuous is not None or posteriors or class_transitions is not None or grammar_posteriors or grammar_continuous is not None
                or grammar_body is not None or grammar_posteriors_body is not None):
            raise ValueError("continuous_posteriors excludes continuous, posteriors, class_transitions, grammar_posteriors, "
                             "grammar_continuous, grammar_body and grammar_posteriors_body")
        with _body_env("ECOZ2_HMM_POSTERIOR_BODY", body):
            check(lib.e2vq_hmm_segment_continuous_files_posteriors(
                m, len(model_filenames), str(codebook).encode() if codebook else None, f, len(input_filenames), int(P), int(W_ms),
                int(O_ms), float(ln_switch), str(continuous_posteriors).encode(), str(csv).encode() if csv else None,
                str(frame_posteriors).encode() if frame_posteriors is not None else None, int(block), int(lookahead)))
        return
    if grammar_body is not None:
        if class_transitions is None:
            raise ValueError("grammar_body needs class_transitions")
        if grammar_posteriors:
            raise ValueError("grammar_body excludes grammar_posteriors (there is one body)")
    if grammar_posteriors_body is not None and not grammar_posteriors:
        raise ValueError("grammar_posteriors_body needs grammar_posteriors=True")
    if grammar_continuous is not None:
        if continuous is not None or posteriors or grammar_posteriors or frame_posteriors is not None or body is not None:
            raise ValueError("grammar_continuous excludes continuous, posteriors, grammar_posteriors, frame_posteriors and body")
        if class_transitions is None:
            raise ValueError("grammar_continuous needs class_transitions")
        with _body_env("ECOZ2_HMM_SEGMENT_TRANS_BODY", grammar_body):
            check(lib.e2vq_hmm_segment_trans_continuous_files(m, len(model_filenames), str(codebook).encode() if codebook else None, f,
                                                              len(input_filenames), int(P), int(W_ms), int(O_ms), float(ln_switch),
                                                              str(class_transitions).encode(), str(grammar_continuous).encode(),
                                                              str(csv).encode() if csv else None))
        return
    if continuous is not None:
        if posteriors or class_transitions is not None or grammar_posteriors:
            raise ValueError("continuous excludes posteriors and class_transitions")
        check(lib.e2vq_hmm_segment_continuous_files(m, len(model_filenames), str(codebook).encode() if codebook else None, f,
                                                    len(input_filenames), int(P), int(W_ms), int(O_ms), float(ln_switch),
                                                    str(continuous).encode(), str(csv).encode() if csv else None))
        return
    if frame_posteriors is not None and not posteriors and not grammar_posteriors:
        raise ValueError("frame_posteriors needs posteriors=True")
    if body is not None and not posteriors:
        raise ValueError("body needs posteriors=True")
    if grammar_posteriors and class_transitions is None:
        raise ValueError("grammar_posteriors needs class_transitions")
    if class_transitions is not None:
        if posteriors:
            raise ValueError("class_transitions and posteriors exclude one another")
        if grammar_posteriors:
            with trans_fb_body(grammar_posteriors_body):
                check(lib.e2vq_hmm_segment_trans_files_posteriors(m, len(model_filenames), str(codebook).encode() if codebook else None, f,
                                                                  len(input_filenames), int(P), int(W_ms), int(O_ms), float(ln_switch),
                                                                  str(class_transitions).encode(), str(csv).encode() if csv else None,
                                                                  str(frame_posteriors).encode() if frame_posteriors is not None else None))
            return
        with _body_env("ECOZ2_HMM_SEGMENT_TRANS_BODY", grammar_body):
            check(lib.e2vq_hmm_segment_trans_files(m, len(model_filenames), str(codebook).encode() if codebook else None, f,
                                                   len(input_filenames), int(P), int(W_ms), int(O_ms), float(ln_switch),
                                                   str(class_transitions).encode(), str(csv).encode() if csv else None))
        return
    if posteriors:
        with _body_env("ECOZ2_HMM_POSTERIOR_BODY", body):
            check(lib.e2vq_hmm_segment_files_posteriors(m, len(model_filenames), str(codebook).encode() if codebook else None, f,
                                                        len(input_filenames), int(P), int(W_ms), int(O_ms), float(ln_switch),
                                                        str(csv).encode() if csv else None,
                                                        str(frame_posteriors).encode() if frame_posteriors is not None else None))
        return
    check(lib.e2vq_hmm_segment_files(m, len(model_filenames), str(codebook).encode() if codebook else None, f,
                                     len(input_filenames), int(P), int(W_ms), int(O_ms), float(ln_switch),
                                     str(csv).encode() if csv else None))


def units_of(units, begin, end, score, ln_switch):
    """the unit table of one aligned stream from its outputs (host arithmetic): a list of dicts unit, cls,
    begin, end (exclusive), score for the units the path visits -- the unit [b, e) scores
    score[e - 1] - (0 if b == 0 else score[b - 1] + ln_switch)"""
    out = []
    ls = np.float64(ln_switch)
    for l, (k, b, e) in enumerate(zip(units, begin, end)):
        if b < 0:
            continue
        with np.errstate(invalid="ignore"):
            lo = np.float64(0.0) if b == 0 else np.float64(score[b - 1]) + ls
            out.append(dict(unit=l, cls=int(k), begin=int(b), end=int(e), score=float(np.float64(score[e - 1]) - lo)))
    return out


def align(models, sym, offs, units, unit_offs, optional=None, ln_switch=0.0, device=0):
    """forced alignment of whole symbol streams to the known order of their units: models = [(pi, A, B)]
    sharing M, each of at most 64 states; sym, offs as `segment` takes them (numpy, or a device tensor); units: class indices,
    the transcript of stream s at units[unit_offs[s]:unit_offs[s + 1]]; optional: a flag per unit (a path may pass over it);
    ln_switch <= 0, finite: the log of the price of a unit boundary.  -> dict: per frame unit / state (uint16), entered
    (uint8), score; per unit begin / end (int64, -1 where the path does not visit it); per stream log_prob, status; and
    units = per stream the list `units_of` gives"""
    a = _transcript_args(models, sym, offs, units, unit_offs, optional, copy=False)
    offs, S, units, unit_offs, nu = a.offs, a.S, a.units, a.unit_offs, a.nu
    n = max(int(offs[-1]), 1)
    unit, state = np.zeros(n, dtype=np.uint16), np.zeros(n, dtype=np.uint16)
    entered, score = np.zeros(n, dtype=np.uint8), np.zeros(n)
    begin, end = np.full(max(nu, 1), -1, dtype=np.int64), np.full(max(nu, 1), -1, dtype=np.int64)
    lp, st = np.zeros(max(S, 1)), np.zeros(max(S, 1), dtype=np.int32)
    check(lib.e2vq_hmm_align(device, *a.c_args, float(ln_switch), unit.ctypes.data, state.ctypes.data, entered.ctypes.data,
                             score.ctypes.data, begin.ctypes.data, end.ctypes.data, lp.ctypes.data, st.ctypes.data, a.on_device))
    T = int(offs[-1])
    out = dict(unit=unit[:T], state=state[:T], entered=entered[:T], score=score[:T], begin=begin[:nu], end=end[:nu], log_prob=lp[:S],
               status=st[:S])
    out["units"] = [units_of(units[ua:ub], begin[ua:ub], end[ua:ub], out["score"][a:b], ln_switch)
                    for a, b, ua, ub in zip(offs[:-1], offs[1:], unit_offs[:-1], unit_offs[1:])]
    return out


def align_last_kernel_ms():
    return _kernel_ms(lib.e2vq_hmm_align_last_kernel_ms)


def align_files(model_filenames, input_filenames, label_filenames, ln_switch=0.0, filler=None, codebook=None, P=36, W_ms=45, O_ms=15,
                csv=None, posteriors=False, frame_posteriors=None, body=None):
    """`hmm align`: input i (.wav, .prd or .seq) aligned to the units label file i names (a segment CSV or a
    selection table, as `hmm transitions` reads them); filler: the class of a model inserted as an optional unit around and
    between them; per input a block on stdout and, with `csv` (a directory, or a .csv file for one input), a CSV of the units.
    posteriors (4.8.12): how sure every unit is, in the block and in five more CSV columns, and with frame_posteriors (a
    directory) a per-frame table for every input; body as `align_posteriors` takes it (it needs posteriors)"""
    if len(label_filenames) != len(input_filenames):
        raise ValueError(f"{len(label_filenames)} label files for {len(input_filenames)} inputs")
    if frame_posteriors is not None and not posteriors:
        raise ValueError("frame_posteriors needs posteriors=True")
    if body is not None and not posteriors:
        raise ValueError("body needs posteriors=True")
    m, _k1 = _strs(model_filenames)
    f, _k2 = _strs(input_filenames)
    l, _k3 = _strs(label_filenames)
    if posteriors:
        with _body_env("ECOZ2_HMM_ALIGN_POSTERIOR_BODY", body):
            check(lib.e2vq_hmm_align_files_posteriors(m, len(model_filenames), str(codebook).encode() if codebook else None, f, l,
                                                      len(input_filenames), int(P), int(W_ms), int(O_ms), float(ln_switch),
                                                      str(filler).encode() if filler else None, str(csv).encode() if csv else None,
                                                      str(frame_posteriors).encode() if frame_posteriors is not None else None))
        return
    check(lib.e2vq_hmm_align_files(m, len(model_filenames), str(codebook).encode() if codebook else None, f, l, len(input_filenames),
                                   int(P), int(W_ms), int(O_ms), float(ln_switch), str(filler).encode() if filler else None,
                                   str(csv).encode() if csv else None))


def align_unit_moments(w0, w1, w2, ref=None):
    """the host arithmetic of DESIGN.md 4.8.12 -> (present, begin_mean, begin_sd); the latter two NaN where not w0 > 0"""
    w0, w1, w2 = (np.ascontiguousarray(x, dtype=np.float64) for x in (w0, w1, w2))
    n = len(w0)
    if len(w1) != n or len(w2) != n or (ref is not None and len(ref) != n):
        raise ValueError("w0, w1, w2 and ref differ in length")
    ref = None if ref is None else np.ascontiguousarray(ref, dtype=np.int64)
    out = [np.zeros(max(n, 1)) for _ in range(3)]
    check(lib.e2vq_hmm_align_unit_moments(n, w0.ctypes.data, w1.ctypes.data, w2.ctypes.data, ref.ctypes.data if ref is not None else None,
                                          out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data))
    return tuple(x[:n] for x in out)


def align_posteriors(models, sym, offs, units, unit_offs, optional=None, ln_switch=0.0, path_unit=None, ref=None, occupancy=True,
                     device=0, body=None):
    """how sure the alignment is: models, sym, offs, units, unit_offs, optional, ln_switch as `align` takes
    them; path_unit: `align`'s per-frame `unit` (or None); ref: a reference frame per unit for the moments (or None = 0)
    -> dict: occ, per stream the (T_s, L_s) array of P(unit l holds frame t) (only with occupancy); post_path per frame (occ at
    the path's unit; 0 without path_unit); per unit w0 = present (P(a path visits the unit)), w1, w2, begin_mean, begin_sd (the
    frame the unit is entered at); per stream log_prob, status.  body: "auto", "resident" or "looped"
    (ECOZ2_HMM_ALIGN_POSTERIOR_BODY for this call: the looped body takes a stream of more than 16 wave-slots, "auto" uses it
    above 16; the same bits either way); None: what the environment says"""
    a = _transcript_args(models, sym, offs, units, unit_offs, optional)
    offs, S, unit_offs, nu = a.offs, a.S, a.unit_offs, a.nu
    T = int(offs[-1])
    if path_unit is not None:
        path_unit = np.ascontiguousarray(path_unit, dtype=np.uint16)
        if len(path_unit) < T:
            raise ValueError(f"path_unit has {len(path_unit)} entries for {T} frames")
    if ref is not None:
        ref = np.ascontiguousarray(ref, dtype=np.int64)
        if len(ref) < nu:
            raise ValueError(f"ref has {len(ref)} entries for {nu} units")
    Ls, Ts = np.diff(unit_offs), np.diff(offs)
    occ_at = np.concatenate([[0], np.cumsum(Ts * Ls)]).astype(np.int64)
    occ = np.zeros(max(int(occ_at[-1]), 1)) if occupancy else None
    post = np.zeros(max(T, 1))
    w0, w1, w2 = (np.zeros(max(nu, 1)) for _ in range(3))
    lp, st = np.zeros(max(S, 1)), np.zeros(max(S, 1), dtype=np.int32)
    with _body_env("ECOZ2_HMM_ALIGN_POSTERIOR_BODY", body):
        check(lib.e2vq_hmm_align_posteriors(device, *a.c_args, float(ln_switch), path_unit.ctypes.data if path_unit is not None else None,
                                            ref.ctypes.data if ref is not None else None, occ.ctypes.data if occ is not None else None,
                                            post.ctypes.data, w0.ctypes.data, w1.ctypes.data, w2.ctypes.data, lp.ctypes.data,
                                            st.ctypes.data, a.on_device))
    present, begin_mean, begin_sd = align_unit_moments(w0[:nu], w1[:nu], w2[:nu], None if ref is None else ref[:nu])
    out = dict(post_path=post[:T], w0=w0[:nu], w1=w1[:nu], w2=w2[:nu], present=present, begin_mean=begin_mean, begin_sd=begin_sd,
               log_prob=lp[:S], status=st[:S])
    if occupancy:
        out["occ"] = [occ[occ_at[s]:occ_at[s + 1]].reshape(int(Ts[s]), int(Ls[s])) for s in range(S)]
    return out


def align_posteriors_last_kernel_ms():
    return _kernel_ms(lib.e2vq_hmm_align_posteriors_last_kernel_ms)


def _transcript_args(models, sym, offs, units, unit_offs, optional, copy=True):
    """the arguments `align`, `align_posteriors`, `embedded_estep` and `train_embedded` share, checked -> a namespace: ms (the
    models' arrays), M, offs, S, units, unit_offs, nu (the units of all streams), on_device (0 / 1), and c_args, what the four
    exports take between `device` and `ln_switch` (it keeps every array alive).  copy: the model arrays are copies
    (train_embedded writes them); without it an array of the right kind is passed as it is"""
    K = len(models)
    arr = (lambda x: np.array(x, dtype=np.float64, order="C")) if copy else (lambda x: np.ascontiguousarray(x, dtype=np.float64))
    ms = [tuple(arr(x) for x in m) for m in models]
    Ns = (C.c_int * max(K, 1))(*[len(m[0]) for m in ms])
    ptrs = [(C.c_void_p * max(K, 1))(*[m[i].ctypes.data for m in ms]) for i in range(3)]
    M = ms[0][2].shape[1] if K else 0
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    unit_offs = np.ascontiguousarray(unit_offs, dtype=np.int64)
    S = len(offs) - 1
    if len(unit_offs) != S + 1:
        raise ValueError(f"unit_offs has {len(unit_offs)} entries for {S} streams")
    units = np.ascontiguousarray(units, dtype=np.int32)
    if optional is not None:
        optional = np.ascontiguousarray(np.asarray(optional) != 0, dtype=np.uint8)
    nu = int(unit_offs[-1]) if len(unit_offs) else 0
    if len(units) < nu or (optional is not None and len(optional) < nu):
        raise ValueError(f"unit_offs ends at {nu}: more than the units given")
    on_device = hasattr(sym, "data_ptr")
    if on_device:
        if not sym.is_contiguous() or sym.element_size() != 2:
            raise ValueError("a device symbol tensor must be contiguous with 2-byte elements")
        sym_ptr = sym.data_ptr()
    else:
        sym = np.ascontiguousarray(sym, dtype=np.uint16)
        sym_ptr = sym.ctypes.data
    c_args = (K, Ns, M, *ptrs, sym_ptr, offs.ctypes.data, S, units.ctypes.data, unit_offs.ctypes.data,
              optional.ctypes.data if optional is not None else None)
    return SimpleNamespace(ms=ms, M=M, offs=offs, S=S, units=units, unit_offs=unit_offs, nu=nu, on_device=int(on_device), c_args=c_args,
                           keep=(optional, sym))


def embedded_estep(models, sym, offs, units, unit_offs, optional=None, ln_switch=0.0, device=0, body=None):
    """one E-step of embedded Baum-Welch: models, sym, offs, units, unit_offs, optional, ln_switch as `align`
    takes them -> dict acc (per class its int64 accumulator words, the layout of `acc_words`), log_prob (ln P(O, transcript)
    per stream, -inf where the status is not 0), status.  body: "auto", "resident" or "looped" (ECOZ2_HMM_EMBED_BODY for this
    call: the looped body takes a stream of more than 16 wave-slots); None: what the environment says"""
    a = _transcript_args(models, sym, offs, units, unit_offs, optional)
    S = a.S
    acc = [np.zeros(int(lib.e2vq_hmm_acc_words(len(m[0]), a.M)), dtype=np.int64) for m in a.ms]
    accp = (C.c_void_p * max(len(acc), 1))(*[x.ctypes.data for x in acc])
    lp, st = np.zeros(max(S, 1)), np.zeros(max(S, 1), dtype=np.int32)
    with _body_env("ECOZ2_HMM_EMBED_BODY", body):
        check(lib.e2vq_hmm_embedded_estep(device, *a.c_args, float(ln_switch), accp, lp.ctypes.data, st.ctypes.data, a.on_device))
    return dict(acc=acc, log_prob=lp[:S], status=st[:S])


def train_embedded(models, sym, offs, units, unit_offs, optional=None, ln_switch=0.0, epsilon=1e-5, val_auto=0.3, max_iterations=-1,
                   device=0, body=None):
    """embedded Baum-Welch to its stop -> (the trained models [(pi, A, B)], the sum of ln P per E-step);
    body as `embedded_estep` takes it"""
    a = _transcript_args(models, sym, offs, units, unit_offs, optional)
    cap = 1000
    hist = np.zeros(cap)
    n = C.c_int(0)
    with _body_env("ECOZ2_HMM_EMBED_BODY", body):
        check(lib.e2vq_hmm_train_embedded(device, *a.c_args, float(ln_switch), float(epsilon), float(val_auto), int(max_iterations),
                                          hist.ctypes.data, cap, C.byref(n), a.on_device))
    return a.ms, hist[:n.value].copy()


def embedded_last_kernel_ms():
    return _kernel_ms(lib.e2vq_hmm_embedded_last_kernel_ms)


def learn_embedded_files(model_filenames, input_filenames, label_filenames, out_dir, ln_switch=0.0, filler=None, hmm_epsilon=1e-5,
                         val_auto=0.3, max_iterations=-1, codebook=None, P=36, W_ms=45, O_ms=15, callback=None, body=None):
    """`hmm learn --embedded`: the models of the files re-estimated from input i (.wav, .prd or .seq) and the
    transcript label file i names (as `align_files` reads it; filler as there); writes <out_dir>/<class>.hmm for every class and
    <out_dir>/embedded.csv; callback(var: str, val: float) per E-step; body as `embedded_estep` takes it"""
    if len(label_filenames) != len(input_filenames):
        raise ValueError(f"{len(label_filenames)} label files for {len(input_filenames)} inputs")
    m, _k1 = _strs(model_filenames)
    f, _k2 = _strs(input_filenames)
    l, _k3 = _strs(label_filenames)
    cb = HMM_LEARN_CALLBACK((lambda v, x: callback(v.decode(), x)) if callback else (lambda _v, _x: None))
    with _body_env("ECOZ2_HMM_EMBED_BODY", body):
        check(lib.e2vq_hmm_learn_embedded_files(m, len(model_filenames), str(codebook).encode() if codebook else None, f, l,
                                                len(input_filenames), int(P), int(W_ms), int(O_ms), float(ln_switch),
                                                str(filler).encode() if filler else None, float(hmm_epsilon), float(val_auto),
                                                int(max_iterations), str(out_dir).encode(), cb))
