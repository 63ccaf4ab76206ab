"""ctypes binding of libbosship.so (include/bosship.h) — the executable twin of the Julia `ccall`
layer described in INTEGRATION.md.  There is NO CPU fallback: if the HIP library is missing or no
GPU is visible, compute calls raise.

Array conventions follow the reference (src/types/data.jl:10-12): X is d×N with one observation
per COLUMN.  numpy arrays are converted to Fortran order so that the memory the C ABI sees is the
same column-major block a Julia Matrix{Float64} would hand to `ccall`.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BOSS_LIB_PATH") or os.path.join(_HERE, "libbosship.so")      # (BOSS_LIB_PATH: A/B timing of another build, tools/)

BOSS_OK, BOSS_E_INVALID, BOSS_E_NO_DEVICE, BOSS_E_NOT_PD, BOSS_E_NEG_VAR, BOSS_E_NOT_FITTED, BOSS_E_ALLOC = range(7)
KERNELS = {"matern32": 0, "matern52": 1, "sqexp": 2}
FIT_NO_SYNC = 1

_c_dp = C.POINTER(C.c_double)
_c_ucp = C.POINTER(C.c_ubyte)

# name -> (restype, argtypes); must list EVERY symbol include/bosship.h declares (tests check it)
SIGNATURES = {
    "boss_version": (C.c_char_p, []),
    "boss_last_error": (C.c_char_p, []),
    "boss_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "boss_set_stream": (C.c_int, [C.c_int, C.c_void_p]),
    "boss_device_sync": (C.c_int, [C.c_int]),
    "boss_gp_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _c_dp, _c_dp, _c_ucp, C.POINTER(C.c_void_p)]),
    "boss_gp_update": (C.c_int, [C.c_void_p, _c_dp, C.c_double, C.c_double, _c_dp, C.c_int, _c_dp]),
    "boss_gp_sync": (C.c_int, [C.c_void_p, _c_dp]),
    "boss_ngp_create": (C.c_int, [C.c_int, C.c_int, C.c_int, _c_dp, _c_dp, _c_ucp, C.POINTER(C.c_void_p)]),
    "boss_ngp_update": (C.c_int, [C.c_void_p, _c_dp, _c_dp, _c_dp, _c_dp, C.c_int, _c_dp]),
    "boss_ngp_predict": (C.c_int, [C.c_void_p, C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, C.POINTER(C.c_long)]),
    "boss_ggp_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _c_dp, _c_dp, _c_dp, C.POINTER(C.c_void_p)]),
    "boss_ggp_update": (C.c_int, [C.c_void_p, _c_dp, C.c_double, C.c_double, C.c_double, C.c_int, _c_dp]),
    "boss_ngp_loglike_grad": (C.c_int, [C.c_void_p, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp]),
    "boss_ngp_append": (C.c_int, [C.c_void_p, C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp]),
    "boss_ngp_reserve": (C.c_int, [C.c_void_p, C.c_int]),
    "boss_ggp_loglike_grad": (C.c_int, [C.c_void_p, _c_dp, _c_dp]),
    "boss_ggp_append": (C.c_int, [C.c_void_p, C.c_int, _c_dp, _c_dp, _c_dp, _c_dp]),
    "boss_ggp_reserve": (C.c_int, [C.c_void_p, C.c_int]),
    "boss_gp_fit": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, C.c_double, C.c_double,
                              _c_ucp, C.POINTER(C.c_void_p), _c_dp]),
    "boss_gp_set_y": (C.c_int, [C.c_void_p, _c_dp]),
    "boss_gp_loglike_grad": (C.c_int, [C.c_void_p, _c_dp, _c_dp]),
    "boss_gp_loglike_grad_mean": (C.c_int, [C.c_void_p, _c_dp, _c_dp, _c_dp]),
    "boss_gp_reserve": (C.c_int, [C.c_void_p, C.c_int]),
    "boss_gp_n": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "boss_gp_append": (C.c_int, [C.c_void_p, C.c_int, _c_dp, _c_dp, _c_dp, _c_dp]),
    "boss_gp_free": (None, [C.c_void_p]),
    "boss_gp_get_factor": (C.c_int, [C.c_void_p, _c_dp, _c_dp]),
    "boss_gp_loglike_batch": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _c_dp, _c_dp, _c_dp, C.c_int, _c_ucp,
                                        C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, C.POINTER(C.c_int)]),
    "boss_gp_loglike_grad_batch": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _c_dp, _c_dp, _c_dp, C.c_int, _c_ucp,
                                             C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, C.POINTER(C.c_int)]),
    "boss_gp_loglike_grad_batch_mean": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _c_dp, _c_dp, _c_dp, C.c_int, _c_ucp,
                                                  C.c_int, _c_dp, _c_dp, _c_dp, C.c_int, _c_dp, C.c_int, _c_dp, _c_dp, _c_dp, _c_dp,
                                                  C.POINTER(C.c_int)]),
    "boss_ggp_loglike_batch": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _c_dp, _c_dp, _c_dp, C.c_int, _c_dp, _c_dp, _c_dp,
                                         _c_dp, _c_dp, C.POINTER(C.c_int)]),
    "boss_ngp_loglike_batch": (C.c_int, [C.c_int, C.c_int, C.c_int, _c_dp, _c_dp, _c_ucp, C.c_int, _c_dp, _c_dp, _c_dp, _c_dp,
                                         C.c_int, _c_dp, C.POINTER(C.c_int)]),
    "boss_ggp_loglike_grad_batch": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _c_dp, _c_dp, _c_dp, C.c_int, _c_dp, _c_dp,
                                              _c_dp, _c_dp, _c_dp, _c_dp, C.POINTER(C.c_int)]),
    "boss_ngp_loglike_grad_batch": (C.c_int, [C.c_int, C.c_int, C.c_int, _c_dp, _c_dp, _c_ucp, C.c_int, _c_dp, _c_dp, _c_dp, _c_dp,
                                              C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, C.POINTER(C.c_int)]),
    "boss_gp_fit_batch": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _c_dp, _c_dp, _c_dp, C.c_int, _c_ucp,
                                    C.c_int, _c_dp, _c_dp, _c_dp, C.POINTER(C.c_void_p), _c_dp, C.POINTER(C.c_int)]),
    "boss_ggp_fit_batch": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _c_dp, _c_dp, _c_dp, C.c_int, _c_dp, _c_dp, _c_dp,
                                     _c_dp, C.POINTER(C.c_void_p), _c_dp, C.POINTER(C.c_int)]),
    "boss_ngp_fit_batch": (C.c_int, [C.c_int, C.c_int, C.c_int, _c_dp, _c_dp, _c_ucp, C.c_int, _c_dp, _c_dp, _c_dp, _c_dp,
                                     C.c_int, C.POINTER(C.c_void_p), _c_dp, C.POINTER(C.c_int)]),
    "boss_ngp_predict_set": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp,
                                       C.POINTER(C.c_long)]),
    "boss_gp_predict": (C.c_int, [C.c_void_p, C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, C.POINTER(C.c_long)]),
    "boss_gp_predict_grad": (C.c_int, [C.c_void_p, C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp,
                                       C.POINTER(C.c_long)]),
    "boss_gp_predict_cov": (C.c_int, [C.c_void_p, C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, C.POINTER(C.c_long)]),
    "boss_ggp_predict_cov": (C.c_int, [C.c_void_p, C.c_int, _c_dp, _c_dp, _c_dp]),
    "boss_ngp_predict_cov": (C.c_int, [C.c_void_p, C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, C.POINTER(C.c_long)]),
    "boss_cand_create": (C.c_int, [C.c_int, C.c_int, C.c_int, _c_dp, C.POINTER(C.c_void_p)]),
    "boss_cand_free": (None, [C.c_void_p]),
    "boss_acq_ei": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_void_p, _c_dp, _c_dp, _c_dp, C.c_int,
                              C.c_double, _c_ucp, _c_dp, C.POINTER(C.c_long), _c_dp]),
    "boss_gp_update_acq": (C.c_int, [C.c_void_p, _c_dp, C.c_double, C.c_double, _c_dp, C.c_void_p, _c_dp, C.c_double, C.c_double,
                                     C.c_int, C.c_double, _c_ucp, _c_dp, _c_dp, _c_dp, _c_dp, C.POINTER(C.c_long), _c_dp,
                                     C.POINTER(C.c_int)]),
    "boss_acq_ei_moments": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, C.c_int,
                                      C.c_double, _c_ucp, _c_dp, C.POINTER(C.c_long), _c_dp]),
    "boss_ngp_predict_grad": (C.c_int, [C.c_void_p, C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp,
                                        C.POINTER(C.c_long)]),
    "boss_acq_ei_grad_moments": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, C.c_int,
                                           C.c_double, _c_ucp, _c_dp, _c_dp]),
    "boss_acq_ei_grad": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, C.c_int,
                                   C.c_double, _c_ucp, _c_dp, _c_dp]),
    "boss_acq_ei_grad_set": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, C.c_int,
                                   C.c_double, _c_ucp, _c_dp, _c_dp]),
    "boss_ngp_predict_grad_set": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp,
                                            _c_dp, _c_dp, _c_dp, _c_dp, C.POINTER(C.c_long)]),
    "boss_ngp_acq_ei_grad_set": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp,
                                           _c_dp, _c_dp, _c_dp, C.c_int, C.c_double, _c_ucp, _c_dp, _c_dp]),
    "boss_nlat_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p), _c_dp, C.c_void_p, C.c_double, C.c_void_p, C.c_double,
                                   C.POINTER(C.c_int), _c_dp, C.POINTER(C.c_int), _c_dp, _c_ucp, C.POINTER(C.c_void_p)]),
    "boss_nlat_free": (None, [C.c_void_p]),
    "boss_nlat_eval": (C.c_int, [C.c_void_p, C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, C.POINTER(C.c_long)]),
    "boss_nfit_create": (C.c_int, [C.c_int, C.c_int, C.c_int, _c_dp, _c_dp, _c_ucp, _c_dp, C.c_int, _c_dp, C.POINTER(C.c_int), _c_dp,
                                   C.POINTER(C.c_int), _c_dp, C.POINTER(C.c_int), _c_dp, C.POINTER(C.c_void_p)]),
    "boss_nfit_free": (None, [C.c_void_p]),
    "boss_nfit_param_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "boss_nfit_values": (C.c_int, [C.c_void_p, C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, C.POINTER(C.c_int)]),
    "boss_nfit_loglike_grad": (C.c_int, [C.c_void_p, C.c_int, _c_dp, _c_dp, _c_dp, C.POINTER(C.c_int)]),
    "boss_ngp_predict_lat": (C.c_int, [C.c_void_p, C.c_int, _c_dp, C.c_void_p, _c_dp, _c_dp, _c_dp, C.POINTER(C.c_long)]),
    "boss_ngp_predict_grad_lat": (C.c_int, [C.c_void_p, C.c_int, _c_dp, C.c_void_p, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp,
                                            C.POINTER(C.c_long)]),
    "boss_ngp_predict_set_lat": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), C.c_int, _c_dp, C.POINTER(C.c_void_p), _c_dp, _c_dp, _c_dp,
                                           C.POINTER(C.c_long)]),
    "boss_ngp_predict_grad_set_lat": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), C.c_int, _c_dp, C.POINTER(C.c_void_p), _c_dp, _c_dp,
                                                _c_dp, _c_dp, _c_dp, _c_dp, C.POINTER(C.c_long)]),
    "boss_ngp_acq_ei_grad_set_lat": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_int, _c_dp, C.POINTER(C.c_void_p), _c_dp,
                                               _c_dp, _c_dp, _c_dp, C.c_int, C.c_double, _c_ucp, _c_dp, _c_dp]),
    "boss_track_create": (C.c_int, [C.c_void_p, C.c_void_p, _c_dp, C.POINTER(C.c_void_p)]),
    "boss_ngp_track_create": (C.c_int, [C.c_void_p, C.c_void_p, _c_dp, _c_dp, _c_dp, C.POINTER(C.c_void_p)]),
    "boss_ngp_track_create_lat": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, _c_dp, C.POINTER(C.c_void_p)]),
    "boss_ggp_track_create": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "boss_track_free": (None, [C.c_void_p]),
    "boss_track_sync": (C.c_int, [C.c_void_p]),
    "boss_track_moments": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _c_dp, _c_dp]),
    "boss_fit_create": (C.c_int, [C.c_int, C.c_int, _c_dp, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]),
    "boss_fit_free": (None, [C.c_void_p]),
    "boss_fit_eval_host": (C.c_int, [C.c_void_p, C.c_int, _c_dp, _c_dp, _c_dp]),
    "boss_acq_ei_mc": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_void_p, _c_dp, C.c_void_p, C.c_int, _c_dp, _c_dp, C.c_int,
                                 C.c_double, _c_ucp, _c_dp, C.POINTER(C.c_long), _c_dp]),
    "boss_acq_ei_mc_moments": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _c_dp, _c_dp, C.c_void_p, C.c_int, _c_dp, _c_dp, C.c_int,
                                         C.c_double, _c_ucp, _c_dp, C.POINTER(C.c_long), _c_dp]),
    "boss_acq_ei_mc_grad": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_int, _c_dp, _c_dp, _c_dp, C.c_void_p, C.c_int, _c_dp,
                                      _c_dp, C.c_int, C.c_double, _c_ucp, _c_dp, _c_dp]),
    "boss_acq_ei_mc_grad_moments": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, C.c_void_p, C.c_int,
                                              _c_dp, _c_dp, C.c_int, C.c_double, _c_ucp, _c_dp, _c_dp]),
    "boss_acqp_create": (C.c_int, [C.c_int, C.c_int, C.c_int, _c_dp, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]),
    "boss_acqp_free": (None, [C.c_void_p]),
    "boss_acqp_eval_host": (C.c_int, [C.c_void_p, C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp]),
    "boss_acq_prog": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_void_p, _c_dp, C.c_void_p, _c_dp, _c_ucp, C.c_double, _c_dp,
                                C.POINTER(C.c_long), _c_dp]),
    "boss_acq_prog_moments": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _c_dp, _c_dp, C.c_void_p, _c_dp, _c_ucp, C.c_double, _c_dp,
                                        C.POINTER(C.c_long), _c_dp]),
    "boss_acq_prog_grad": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_int, _c_dp, _c_dp, _c_dp, C.c_void_p, _c_dp, _c_ucp,
                                     C.c_double, _c_dp, _c_dp]),
    "boss_acq_prog_grad_moments": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, C.c_void_p, _c_dp,
                                             _c_ucp, C.c_double, _c_dp, _c_dp]),
    "boss_mean_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), _c_dp, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                   C.POINTER(C.c_int), C.POINTER(C.c_void_p)]),
    "boss_mean_free": (None, [C.c_void_p]),
    "boss_mean_eval_host": (C.c_int, [C.c_void_p, C.c_int, _c_dp, C.c_int, _c_dp, C.c_int, _c_dp, _c_dp, _c_dp]),
    "boss_mean_eval": (C.c_int, [C.c_int, C.c_void_p, C.c_int, _c_dp, C.c_int, _c_dp, C.c_int, _c_dp, _c_dp, _c_dp]),
    "boss_kern_create": (C.c_int, [C.c_int, C.c_int, _c_dp, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]),
    "boss_kern_free": (None, [C.c_void_p]),
    "boss_kern_eval_host": (C.c_int, [C.c_void_p, C.c_int, _c_dp, _c_dp, _c_dp]),
    "boss_kgp_create": (C.c_int, [C.c_int, C.c_int, C.c_int, _c_dp, _c_dp, _c_ucp, C.c_void_p, C.POINTER(C.c_void_p)]),
    "boss_kern_grad_host": (C.c_int, [C.c_void_p, C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp]),
    "boss_kgp_set_grad": (C.c_int, [C.c_void_p, C.c_int]),
    "boss_kgp_set_sequential": (C.c_int, [C.c_void_p, C.c_int]),
    "boss_kgp_loglike_batch": (C.c_int, [C.c_int, C.c_int, C.c_int, _c_dp, _c_dp, _c_ucp, C.c_void_p, C.c_int, _c_dp, _c_dp, _c_dp, _c_dp,
                                         C.c_int, _c_dp, C.POINTER(C.c_int)]),
    "boss_kgp_fit_batch": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, _c_dp, _c_dp, _c_dp, C.c_int, _c_ucp, C.c_int, _c_dp, _c_dp,
                                     _c_dp, C.POINTER(C.c_void_p), _c_dp, C.POINTER(C.c_int)]),
    "boss_warp_create": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "boss_warp_free": (None, [C.c_void_p]),
    "boss_warp_apply_host": (C.c_int, [C.c_void_p, C.c_int, _c_dp, _c_dp, _c_dp]),
    "boss_warp_apply": (C.c_int, [C.c_int, C.c_void_p, C.c_int, _c_dp, _c_dp, _c_dp]),
    "boss_warp_moments_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp,
                                         _c_dp, C.POINTER(C.c_long)]),
    "boss_warp_moments": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp,
                                    _c_dp, _c_dp, C.POINTER(C.c_long)]),
    "boss_warp_predict": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_int, _c_dp, _c_dp, _c_dp, _c_dp,
                                    C.POINTER(C.c_long)]),
    "boss_warp_predict_grad": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp,
                                         _c_dp, _c_dp, C.POINTER(C.c_long)]),
    "boss_acq_ei_warp": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, C.c_int,
                                   C.c_double, _c_ucp, _c_dp, C.POINTER(C.c_long), _c_dp]),
    "boss_acq_ei_grad_warp": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp,
                                        C.c_int, C.c_double, _c_ucp, _c_dp, _c_dp]),
    "boss_acq_ei_tracks": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p), _c_dp, _c_dp, C.c_int, C.c_double, _c_ucp,
                                     _c_dp, C.POINTER(C.c_long), _c_dp]),
    "boss_init": (C.c_int, [C.POINTER(C.c_int)]),
    "boss_comm_info": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "boss_shutdown": (None, []),
    "boss_multi_gp_update": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), _c_dp, C.c_double, C.c_double, _c_dp, _c_dp]),
    "boss_multi_acq_ei": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, C.c_int,
                                    C.c_double, _c_ucp, _c_dp, C.POINTER(C.c_long), _c_dp]),
    "boss_multi_cand_create": (C.c_int, [C.c_int, C.c_int, C.c_int, _c_dp, C.POINTER(C.c_void_p)]),
    "boss_multi_cand_free": (None, [C.c_void_p]),
    "boss_multi_acq_ei_cand": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_void_p, _c_dp, _c_dp, _c_dp, C.c_int,
                                         C.c_double, _c_ucp, _c_dp, C.POINTER(C.c_long), _c_dp]),
    "boss_multi_acq_ei_outputs": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, C.c_int,
                                            C.c_double, _c_ucp, _c_dp, C.POINTER(C.c_long), _c_dp]),
    "boss_multi_acq_ei_samples": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_int, _c_dp, _c_dp, _c_dp, _c_dp, C.c_int,
                                            C.c_double, _c_ucp, _c_dp, C.POINTER(C.c_long), _c_dp]),
    "boss_multi_loglike_batch": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _c_dp, _c_dp, _c_dp, C.c_int, _c_ucp, C.c_int,
                                           _c_dp, _c_dp, _c_dp, _c_dp, C.POINTER(C.c_int)]),
    "boss_bench_mfma_f64": (C.c_int, [C.c_int, C.c_int, _c_dp]),
    "boss_prof_enable": (C.c_int, [C.c_int, C.c_int]),
    "boss_prof_reset": (C.c_int, [C.c_int]),
    "boss_prof_get": (C.c_int, [C.c_int, C.c_char_p, _c_dp, C.POINTER(C.c_long)]),
}


class BossError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[bosship status {code}] {msg}")
        self.code = code


class PosDefException(BossError):
    """LinearAlgebra.PosDefException analogue (BOSS_E_NOT_PD)."""


class DomainError(BossError):
    """DomainError of `_clip_var` (src/models/gaussian_process.jl:186-194) (BOSS_E_NEG_VAR)."""

    bad_index: int = -1


_lib = None


def load_library(path: Optional[str] = None):
    """dlopen libbosship.so and attach prototypes.  Raises if the library was not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise FileNotFoundError(
            f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(bosship has no CPU fallback)")
    lib = C.CDLL(p)
    for name, (res, args) in SIGNATURES.items():
        if os.environ.get("BOSS_LIB_PATH") and not hasattr(lib, name):
            continue                                   # (an older build under A/B timing lacks the newer entry points)
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _check(rc: int):
    if rc == BOSS_OK:
        return
    msg = load_library().boss_last_error().decode()
    if rc == BOSS_E_NOT_PD:
        raise PosDefException(rc, msg)
    if rc == BOSS_E_NEG_VAR:
        raise DomainError(rc, msg)
    raise BossError(rc, msg)


def _f64(a, ndim=None):
    a = np.asfortranarray(a, dtype=np.float64)
    if ndim is not None and a.ndim != ndim:
        raise ValueError(f"expected a {ndim}-d array, got shape {a.shape}")
    return a


def _dp(a):
    return None if a is None else a.ctypes.data_as(_c_dp)


def _ucp(a):
    return None if a is None else a.ctypes.data_as(_c_ucp)


def _kernel_id(kernel) -> int:
    return KERNELS[kernel] if isinstance(kernel, str) else int(kernel)


def device_count() -> int:
    n = C.c_int(0)
    load_library().boss_device_count(C.byref(n))
    return n.value


def set_stream(device: int, stream_ptr: Optional[int]):
    _check(load_library().boss_set_stream(device, C.c_void_p(stream_ptr or 0)))


def device_sync(device: int = 0):
    _check(load_library().boss_device_sync(device))


class GP:
    """One output slice's posterior, resident on a GPU (boss_gp_t)."""

    def __init__(self, X, y, kernel="matern52", discrete=None, device: int = 0):
        lib = load_library()
        X = _f64(X, 2)
        y = _f64(np.asarray(y).reshape(-1), 1)
        self.d, self.N = X.shape
        if y.shape[0] != self.N:
            raise ValueError("y must have one entry per column of X")
        self.device = device
        self.kernel = _kernel_id(kernel)
        disc = None if discrete is None else np.ascontiguousarray(np.asarray(discrete, dtype=bool).astype(np.uint8))
        h = C.c_void_p()
        _check(lib.boss_gp_create(device, self.kernel, self.d, self.N, _dp(X), _dp(y), _ucp(disc), C.byref(h)))
        self._h = h
        self.logpdf = None

    def update(self, lengthscale, amplitude, noise_std, mean_X=None, sync: bool = True) -> Optional[float]:
        lib = load_library()
        lam = _f64(np.asarray(lengthscale).reshape(-1), 1)
        if lam.shape[0] != self.d:
            # gaussian_process.jl:233 @assert length(lengthscales) == size(X, 1)
            raise BossError(BOSS_E_INVALID, "length(lengthscales) must equal x_dim")
        m = None if mean_X is None else _f64(np.asarray(mean_X).reshape(-1), 1)
        if m is not None and m.shape[0] != self.N:
            raise ValueError("mean_X must have N entries")
        out = C.c_double(0.0)
        rc = lib.boss_gp_update(self._h, _dp(lam), float(amplitude), float(noise_std), _dp(m),
                                0 if sync else FIT_NO_SYNC, C.byref(out))
        _check(rc)
        if sync:
            self.logpdf = out.value
            return out.value
        return None

    def update_acq(self, lengthscale, amplitude, noise_std, cand: "Candidates", fit_coef: float = 1.0, y_max: Optional[float] = None,
                   best=None, mean_X=None, mean_Xs=None, valid_mask=None, want_acq: bool = False, want_moments: bool = False):
        """One BO iteration's posterior update with its first acquisition riding along the factorisation
        (boss_gp_update_acq): `update` followed by `acq_ei([[self]], cand, [fit_coef], [y_max], best)` in one call
        (y_max None: `constraints === nothing`; +Inf: a constraint that always holds).
        Returns a dict: logpdf, argmax, max, fused (True when the substitution rode along), and acq / mu / var on request
        (mu, var unclipped)."""
        lam = _f64(np.asarray(lengthscale).reshape(-1), 1)
        if lam.shape[0] != self.d:
            raise BossError(BOSS_E_INVALID, "length(lengthscales) must equal x_dim")
        m = None if mean_X is None else _f64(np.asarray(mean_X).reshape(-1), 1)
        if m is not None and m.shape[0] != self.N:
            raise ValueError("mean_X must have N entries")
        M = cand.M
        ms = None if mean_Xs is None else _f64(np.asarray(mean_Xs).reshape(-1), 1)
        if ms is not None and ms.shape[0] != M:
            raise ValueError("mean_Xs must have one entry per candidate")
        mask = None if valid_mask is None else np.ascontiguousarray(np.asarray(valid_mask, dtype=bool).astype(np.uint8))
        if mask is not None and mask.shape[0] != M:
            raise ValueError("valid_mask must have one entry per candidate")
        acq = np.zeros(M) if want_acq else None
        mu = np.zeros(M) if want_moments else None
        var = np.zeros(M) if want_moments else None
        lp, am, mx, fused = C.c_double(0.0), C.c_long(-1), C.c_double(0.0), C.c_int(0)
        _check(load_library().boss_gp_update_acq(self._h, _dp(lam), float(amplitude), float(noise_std), _dp(m), cand._h, _dp(ms),
                                                 float(fit_coef), float("nan") if y_max is None else float(y_max), 0 if best is None else 1,
                                                 0.0 if best is None else float(best), _ucp(mask), C.byref(lp), _dp(mu), _dp(var),
                                                 _dp(acq), C.byref(am), C.byref(mx), C.byref(fused)))
        self.logpdf = lp.value
        return {"logpdf": lp.value, "argmax": am.value, "max": mx.value, "fused": bool(fused.value), "acq": acq, "mu": mu, "var": var}

    def sync(self) -> float:
        out = C.c_double(0.0)
        _check(load_library().boss_gp_sync(self._h, C.byref(out)))
        self.logpdf = out.value
        return out.value

    def set_y(self, y):
        y = _f64(np.asarray(y).reshape(-1), 1)
        _check(load_library().boss_gp_set_y(self._h, _dp(y)))

    def loglike_grad(self):
        """(logpdf, grad[d+2]) at the hyper-parameters of the last update: gradient w.r.t.
        (lengthscale[d], amplitude, noise_std), analytic, on the device."""
        out = C.c_double(0.0)
        grad = np.zeros(self.d + 2)
        _check(load_library().boss_gp_loglike_grad(self._h, C.byref(out), _dp(grad)))
        return out.value, grad

    def loglike_grad_mean(self):
        """(logpdf, grad[d+2], dmean[N]): loglike_grad plus ∂logpdf/∂(prior mean value at x_j) = (K⁻¹(y − m))_j at the handle's current N
        observations.  With the Jacobian J (N×T) of the mean values w.r.t. the parameters θ of a parametric mean, ∂logpdf/∂θ = Jᵀ dmean."""
        lib = load_library()
        n = C.c_int(0)
        _check(lib.boss_gp_n(self._h, C.byref(n)))
        out = C.c_double(0.0)
        grad = np.zeros(self.d + 2)
        dmean = np.zeros(n.value)
        _check(lib.boss_gp_loglike_grad_mean(self._h, C.byref(out), _dp(grad), _dp(dmean)))
        return out.value, grad, dmean

    def reserve(self, N_total: int):
        """Reserve storage for N_total observations (later appends need no re-allocation); the handle
        must be (re-)updated afterwards."""
        _check(load_library().boss_gp_reserve(self._h, int(N_total)))

    def append(self, X_new, y_new, mean_new=None) -> float:
        """augment_dataset! + model_posterior with unchanged hyper-parameters (block Cholesky
        append): X_new d×n (or a length-d vector), y_new n.  Returns the logpdf of all N+n points."""
        X_new = _f64(X_new)
        if X_new.ndim == 1:
            X_new = _f64(X_new.reshape(-1, 1))
        if X_new.shape[0] != self.d:
            raise ValueError("X_new must be d×n")
        n = X_new.shape[1]
        y_new = _f64(np.asarray(y_new).reshape(-1), 1)
        if y_new.shape[0] != n:
            raise ValueError("y_new must have one entry per new point")
        m = None if mean_new is None else _f64(np.asarray(mean_new).reshape(-1), 1)
        if m is not None and m.shape[0] != n:
            raise ValueError("mean_new must have one entry per new point")
        out = C.c_double(0.0)
        rc = load_library().boss_gp_append(self._h, n, _dp(X_new), _dp(y_new), _dp(m), C.byref(out))
        cnt = C.c_int(self.N)                # the device's own count: observations stay appended when the factorisation
        load_library().boss_gp_n(self._h, C.byref(cnt))   # fails, and a failed multi-append may have taken only some
        self.N = cnt.value
        _check(rc)
        self.logpdf = out.value
        return out.value

    def factor(self):
        L = np.zeros((self.N, self.N), order="F")
        z = np.zeros(self.N)
        _check(load_library().boss_gp_get_factor(self._h, _dp(L), _dp(z)))
        return L, z

    def predict(self, Xs, mean_Xs=None):
        """mean_and_var(post, X::Matrix): returns (mu[M], var[M]) with _clip_var applied."""
        Xs = _f64(Xs)
        if Xs.ndim == 1:
            Xs = _f64(Xs.reshape(-1, 1))
        if Xs.shape[0] != self.d:
            raise ValueError("candidates must be d×M")
        M = Xs.shape[1]
        ms = None if mean_Xs is None else _f64(np.asarray(mean_Xs).reshape(-1), 1)
        mu = np.zeros(M)
        var = np.zeros(M)
        bad = C.c_long(-1)
        rc = load_library().boss_gp_predict(self._h, M, _dp(Xs), _dp(ms), _dp(mu), _dp(var), C.byref(bad))
        if rc == BOSS_E_NEG_VAR:
            e = DomainError(rc, load_library().boss_last_error().decode())
            e.bad_index = bad.value
            raise e
        _check(rc)
        return mu, var

    def predict_grad(self, Xs, mean_Xs=None, mean_grad=None):
        """mean_and_var(post, X) and its gradient w.r.t. the candidates: returns
        (mu[M], var[M], dmu[d,M], dvar[d,M]) — analytic, evaluated on the device."""
        Xs = _f64(Xs)
        if Xs.ndim == 1:
            Xs = _f64(Xs.reshape(-1, 1))
        if Xs.shape[0] != self.d:
            raise ValueError("candidates must be d×M")
        M = Xs.shape[1]
        ms = None if mean_Xs is None else _f64(np.asarray(mean_Xs).reshape(-1), 1)
        mg = None if mean_grad is None else _f64(mean_grad, 2)
        if mg is not None and mg.shape != (self.d, M):
            raise ValueError("mean_grad must be d×M")
        mu, var = np.zeros(M), np.zeros(M)
        dmu, dvar = np.zeros((self.d, M), order="F"), np.zeros((self.d, M), order="F")
        bad = C.c_long(-1)
        rc = load_library().boss_gp_predict_grad(self._h, M, _dp(Xs), _dp(ms), _dp(mg), _dp(mu), _dp(var), _dp(dmu),
                                                 _dp(dvar), C.byref(bad))
        if rc == BOSS_E_NEG_VAR:
            e = DomainError(rc, load_library().boss_last_error().decode())
            e.bad_index = bad.value
            raise e
        _check(rc)
        return mu, var, dmu, dvar

    def predict_cov(self, Xs, mean_Xs=None):
        """mean_and_cov(post, X::Matrix): returns (mu[M], cov[M,M]) with the diagonal clipped."""
        Xs = _f64(Xs, 2)
        if Xs.shape[0] != self.d:
            raise ValueError("candidates must be d×M")
        M = Xs.shape[1]
        ms = None if mean_Xs is None else _f64(np.asarray(mean_Xs).reshape(-1), 1)
        mu = np.zeros(M)
        cov = np.zeros((M, M), order="F")
        bad = C.c_long(-1)
        rc = load_library().boss_gp_predict_cov(self._h, M, _dp(Xs), _dp(ms), _dp(mu), _dp(cov), C.byref(bad))
        if rc == BOSS_E_NEG_VAR:
            e = DomainError(rc, load_library().boss_last_error().decode())
            e.bad_index = bad.value
            raise e
        _check(rc)
        return mu, cov

    def close(self):
        if getattr(self, "_h", None):
            load_library().boss_gp_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GradGP(GP):
    """One output slice's posterior conditioned on values AND gradients (GradientGaussianProcess,
    src/models/gradient_gp.jl): X d×n, y n, dY d×n.  `N` is the size of the augmented system n(1+d)."""

    def __init__(self, X, y, dY, kernel="matern52", device: int = 0):
        lib = load_library()
        X = _f64(X, 2)
        y = _f64(np.asarray(y).reshape(-1), 1)
        dY = np.asfortranarray(np.asarray(dY, dtype=np.float64))
        self.d, self.n = X.shape
        if y.shape[0] != self.n or dY.shape != (self.d, self.n):
            raise ValueError("y must have n entries and dY must be d×n")
        self.N = self.n * (1 + self.d)
        self.device = device
        self.kernel = _kernel_id(kernel)
        h = C.c_void_p()
        _check(lib.boss_ggp_create(device, self.kernel, self.d, self.n, _dp(X), _dp(y),
                                   dY.ctypes.data_as(_c_dp), C.byref(h)))
        self._h = h
        self.logpdf = None

    def update(self, lengthscale, amplitude, noise_std, grad_noise_std, sync: bool = True) -> Optional[float]:
        lam = _f64(np.asarray(lengthscale).reshape(-1), 1)
        if lam.shape[0] != self.d:
            raise BossError(BOSS_E_INVALID, "length(lengthscales) must equal x_dim")
        out = C.c_double(0.0)
        _check(load_library().boss_ggp_update(self._h, _dp(lam), float(amplitude), float(noise_std), float(grad_noise_std),
                                              0 if sync else FIT_NO_SYNC, C.byref(out)))
        if sync:
            self.logpdf = out.value
            return out.value
        return None

    def loglike_grad(self):
        """(logpdf, grad[d+3]) at the parameters of the last update: gradient w.r.t. (lengthscale[d], amplitude, noise_std,
        grad_noise_std) — what ForwardDiff yields through data_loglike (gradient_gp.jl:367-397) inside OptimizationMAP."""
        out = C.c_double(0.0)
        grad = np.zeros(self.d + 3)
        _check(load_library().boss_ggp_loglike_grad(self._h, C.byref(out), _dp(grad)))
        return out.value, grad

    def reserve(self, N_total=None, *, points: Optional[int] = None):
        """Reserve storage for `points` POINTS in all, points (1 + d) rows (boss_ggp_reserve); the handle must be (re-)updated
        afterwards.  The count is named: GP.reserve's positional N_total counts observations, which this model has 1 + d of per
        point, and stays refused as boss_gp_reserve refuses these handles."""
        if N_total is not None or points is None:
            raise BossError(BOSS_E_INVALID, "a gradient-observation posterior reserves in points: reserve(points=n_points_total)")
        _check(load_library().boss_ggp_reserve(self._h, int(points)))

    def append(self, X_new, y_new, dY_new) -> float:
        """augment_dataset! + the posterior at unchanged hyper-parameters: X_new d×m (or a length-d vector), y_new m, dY_new d×m.
        The 1 + d rows of every new point go to the end of the handle's own ordering and the block rows of the factor that hold
        them are rebuilt on the device (boss_ggp_append).  Returns the logpdf of all n + m points."""
        X_new = _f64(np.asarray(X_new, dtype=np.float64).reshape(self.d, -1), 2)
        m = X_new.shape[1]
        y_new = _f64(np.asarray(y_new).reshape(-1), 1)
        dY_new = np.asfortranarray(np.asarray(dY_new, dtype=np.float64).reshape(self.d, -1))
        if y_new.shape[0] != m or dY_new.shape != (self.d, m):
            raise ValueError("y_new must have one entry and dY_new one column per new point")
        out = C.c_double(0.0)
        rc = load_library().boss_ggp_append(self._h, m, _dp(X_new), _dp(y_new), dY_new.ctypes.data_as(_c_dp), C.byref(out))
        cnt = C.c_int(self.N)                # the device's own count: the points stay appended when the factorisation fails
        load_library().boss_gp_n(self._h, C.byref(cnt))
        self.N = cnt.value
        self.n = self.N // (1 + self.d)
        _check(rc)
        self.logpdf = out.value
        return out.value

    def predict_value_cov(self, Xs):
        """mean_and_cov of the value posterior (gradient_gp.jl:368-373, boss_ggp_predict_cov): returns (mu[M], cov[M,M]),
        cov exactly symmetric, neither jittered nor clipped."""
        Xs = _f64(Xs)
        if Xs.ndim == 1:
            Xs = _f64(Xs.reshape(-1, 1))
        if Xs.shape[0] != self.d:
            raise ValueError("candidates must be d×M")
        M = Xs.shape[1]
        mu = np.zeros(M)
        cov = np.zeros((M, M), order="F")
        _check(load_library().boss_ggp_predict_cov(self._h, M, _dp(Xs), _dp(mu), _dp(cov)))
        return mu, cov


class GibbsGP(GP):
    """One output slice's posterior under the NonstationaryGP's Gibbs kernel (nonstationary_gp.jl:61-107): the
    latent λ(·), α(·), σ(·) are evaluated by the caller and passed as arrays."""

    def __init__(self, X, y, discrete=None, device: int = 0):
        lib = load_library()
        X = _f64(X, 2)
        y = _f64(np.asarray(y).reshape(-1), 1)
        self.d, self.N = X.shape
        if y.shape[0] != self.N:
            raise ValueError("y must have one entry per column of X")
        self.device = device
        self.kernel = None
        disc = None if discrete is None else np.ascontiguousarray(np.asarray(discrete, dtype=bool).astype(np.uint8))
        h = C.c_void_p()
        _check(lib.boss_ngp_create(device, self.d, self.N, _dp(X), _dp(y), _ucp(disc), C.byref(h)))
        self._h = h
        self.logpdf = None

    def update(self, lam_X, amp_X, noise_X, mean_X=None, sync: bool = True) -> Optional[float]:
        lam = _f64(lam_X, 2)
        amp = _f64(np.asarray(amp_X).reshape(-1), 1)
        noi = _f64(np.asarray(noise_X).reshape(-1), 1)
        if lam.shape != (self.d, self.N) or amp.shape[0] != self.N or noi.shape[0] != self.N:
            raise ValueError("lam_X must be d×N, amp_X and noise_X length N")
        m = None if mean_X is None else _f64(np.asarray(mean_X).reshape(-1), 1)
        if m is not None and m.shape[0] != self.N:
            raise ValueError("mean_X must have N entries")
        out = C.c_double(0.0)
        _check(load_library().boss_ngp_update(self._h, _dp(lam), _dp(amp), _dp(noi), _dp(m), 0 if sync else FIT_NO_SYNC,
                                              C.byref(out)))
        if sync:
            self.logpdf = out.value
            return out.value
        return None

    def loglike_grad(self):
        """(logpdf, dlam[d, N], damp[N], dnoise[N], dmean[N]): the log-likelihood of the last update and its partial derivatives w.r.t.
        the latent models' values at the training points (boss_ngp_loglike_grad)."""
        out = C.c_double(0.0)
        dlam = np.zeros((self.d, self.N), order="F")
        damp, dnoi, dmean = np.zeros(self.N), np.zeros(self.N), np.zeros(self.N)
        _check(load_library().boss_ngp_loglike_grad(self._h, C.byref(out), _dp(dlam), _dp(damp), _dp(dnoi), _dp(dmean)))
        return out.value, dlam, damp, dnoi, dmean

    def reserve(self, N_total: int):
        """Reserve storage for N_total observations (boss_ngp_reserve); the handle must be (re-)updated afterwards, with latent
        arrays of N columns as before."""
        _check(load_library().boss_ngp_reserve(self._h, int(N_total)))

    def append(self, X_new, y_new, lam_new, amp_new, noise_new, mean_new=None) -> float:
        """augment_dataset! + the posterior with the latent models evaluated at the new points (lam_new d×m, amp_new m, noise_new m):
        the block rows of the factor that hold the new points are rebuilt on the device (boss_ngp_append).  Returns the logpdf of
        all N + m points."""
        X_new = _f64(np.asarray(X_new, dtype=np.float64).reshape(self.d, -1), 2)
        m = X_new.shape[1]
        y_new = _f64(np.asarray(y_new).reshape(-1), 1)
        lam = _f64(np.asarray(lam_new, dtype=np.float64).reshape(self.d, -1), 2)
        amp = _f64(np.asarray(amp_new).reshape(-1), 1)
        noi = _f64(np.asarray(noise_new).reshape(-1), 1)
        mn = None if mean_new is None else _f64(np.asarray(mean_new).reshape(-1), 1)
        if y_new.shape[0] != m or lam.shape != (self.d, m) or amp.shape[0] != m or noi.shape[0] != m or (mn is not None and mn.shape[0] != m):
            raise ValueError("one entry (column) per new point in y_new, lam_new, amp_new, noise_new, mean_new")
        out = C.c_double(0.0)
        rc = load_library().boss_ngp_append(self._h, m, _dp(X_new), _dp(y_new), _dp(lam), _dp(amp), _dp(noi), _dp(mn), C.byref(out))
        cnt = C.c_int(self.N)                # the device's own count: the observations stay appended when the factorisation fails
        load_library().boss_gp_n(self._h, C.byref(cnt))
        self.N = cnt.value
        _check(rc)
        self.logpdf = out.value
        return out.value

    def predict(self, Xs, lam_Xs, amp_Xs, mean_Xs=None):
        """mean_and_var with _clip_var; lam_Xs d×M and amp_Xs M are λ(x*), α(x*)."""
        Xs = _f64(Xs)
        if Xs.ndim == 1:
            Xs = _f64(Xs.reshape(-1, 1))
        M = Xs.shape[1]
        lam = _f64(np.asarray(lam_Xs, dtype=np.float64).reshape(self.d, M), 2)
        amp = _f64(np.asarray(amp_Xs).reshape(-1), 1)
        if Xs.shape[0] != self.d or amp.shape[0] != M:
            raise ValueError("candidates must be d×M with lam_Xs d×M and amp_Xs M")
        ms = None if mean_Xs is None else _f64(np.asarray(mean_Xs).reshape(-1), 1)
        mu = np.zeros(M)
        var = np.zeros(M)
        bad = C.c_long(-1)
        rc = load_library().boss_ngp_predict(self._h, M, _dp(Xs), _dp(lam), _dp(amp), _dp(ms), _dp(mu), _dp(var), C.byref(bad))
        if rc == BOSS_E_NEG_VAR:
            e = DomainError(rc, load_library().boss_last_error().decode())
            e.bad_index = bad.value
            raise e
        _check(rc)
        return mu, var

    def predict_cov(self, Xs, lam_Xs=None, amp_Xs=None, mean_Xs=None):
        """mean_and_cov with the diagonal through _clip_var (boss_ngp_predict_cov): returns (mu[M], cov[M,M]); lam_Xs d×M and
        amp_Xs M are λ(x*), α(x*) at the (rounded) candidates.  Without them the library refuses the call (BossError)."""
        Xs = _f64(Xs)
        if Xs.ndim == 1:
            Xs = _f64(Xs.reshape(-1, 1))
        if Xs.shape[0] != self.d:
            raise ValueError("candidates must be d×M")
        M = Xs.shape[1]
        lam = None if lam_Xs is None else _f64(np.asarray(lam_Xs, dtype=np.float64).reshape(self.d, M), 2)
        amp = None if amp_Xs is None else _f64(np.asarray(amp_Xs).reshape(-1), 1)
        if amp is not None and amp.shape[0] != M:
            raise ValueError("amp_Xs must have M entries")
        ms = None if mean_Xs is None else _f64(np.asarray(mean_Xs).reshape(-1), 1)
        mu = np.zeros(M)
        cov = np.zeros((M, M), order="F")
        bad = C.c_long(-1)
        rc = load_library().boss_ngp_predict_cov(self._h, M, _dp(Xs), _dp(lam), _dp(amp), _dp(ms), _dp(mu), _dp(cov), C.byref(bad))
        if rc == BOSS_E_NEG_VAR:
            e = DomainError(rc, load_library().boss_last_error().decode())
            e.bad_index = bad.value
            raise e
        _check(rc)
        return mu, cov

    def predict_grad(self, Xs, lam_Xs, amp_Xs, dlam_Xs=None, damp_Xs=None, mean_Xs=None, mean_grad=None):
        """mean_and_var and its gradient w.r.t. the candidates (boss_ngp_predict_grad): dlam_Xs d×d×M with [l, m, j] = ∂λ_l/∂x_m at
        candidate j (None: constant λ), damp_Xs d×M (None: constant α).  Returns (mu[M], var[M], dmu[d,M], dvar[d,M])."""
        Xs = _f64(Xs)
        if Xs.ndim == 1:
            Xs = _f64(Xs.reshape(-1, 1))
        M = Xs.shape[1]
        lam = _f64(np.asarray(lam_Xs, dtype=np.float64).reshape(self.d, M), 2)
        amp = _f64(np.asarray(amp_Xs).reshape(-1), 1)
        if Xs.shape[0] != self.d or amp.shape[0] != M:
            raise ValueError("candidates must be d×M with lam_Xs d×M and amp_Xs M")
        dl = None if dlam_Xs is None else np.asfortranarray(np.asarray(dlam_Xs, dtype=np.float64).reshape(self.d, self.d, M))
        da = None if damp_Xs is None else _f64(np.asarray(damp_Xs, dtype=np.float64).reshape(self.d, M), 2)
        ms = None if mean_Xs is None else _f64(np.asarray(mean_Xs).reshape(-1), 1)
        mg = None if mean_grad is None else _f64(np.asarray(mean_grad, dtype=np.float64).reshape(self.d, M), 2)
        mu, var = np.zeros(M), np.zeros(M)
        dmu, dvar = np.zeros((self.d, M), order="F"), np.zeros((self.d, M), order="F")
        bad = C.c_long(-1)
        rc = load_library().boss_ngp_predict_grad(self._h, M, _dp(Xs), _dp(lam), _dp(amp), _dp(dl), _dp(da), _dp(ms), _dp(mg), _dp(mu),
                                                  _dp(var), _dp(dmu), _dp(dvar), C.byref(bad))
        if rc == BOSS_E_NEG_VAR:
            e = DomainError(rc, load_library().boss_last_error().decode())
            e.bad_index = bad.value
            raise e
        _check(rc)
        return mu, var, dmu, dvar

    def _lat_args(self, Xs, lat, mean_Xs, mean_grad=None):
        Xs = _f64(Xs)
        if Xs.ndim == 1:
            Xs = _f64(Xs.reshape(-1, 1))
        if Xs.ndim != 2 or Xs.shape[0] != self.d:
            raise ValueError("candidates must be d×M")
        if not isinstance(lat, NgpLatents) or lat._h is None:
            raise BossError(BOSS_E_INVALID, "lat must be an open NgpLatents")
        M = Xs.shape[1]
        ms = None if mean_Xs is None else _f64(np.asarray(mean_Xs).reshape(-1), 1)
        mg = None if mean_grad is None else _f64(np.asarray(mean_grad, dtype=np.float64).reshape(self.d, M), 2)
        return Xs, M, ms, mg

    def predict_lat(self, Xs, lat: "NgpLatents", mean_Xs=None):
        """predict with λ(x*), α(x*) read from the resident latent models `lat` on the device (boss_ngp_predict_lat)."""
        Xs, M, ms, _ = self._lat_args(Xs, lat, mean_Xs)
        mu, var = np.zeros(M), np.zeros(M)
        bad = C.c_long(-1)
        rc = load_library().boss_ngp_predict_lat(self._h, M, _dp(Xs), lat._h, _dp(ms), _dp(mu), _dp(var), C.byref(bad))
        if rc == BOSS_E_NEG_VAR:
            e = DomainError(rc, load_library().boss_last_error().decode())
            e.bad_index = bad.value
            raise e
        _check(rc)
        return mu, var

    def predict_grad_lat(self, Xs, lat: "NgpLatents", mean_Xs=None, mean_grad=None):
        """predict_grad with the latent values and their analytic Jacobians read from `lat` on the device
        (boss_ngp_predict_grad_lat).  Returns (mu[M], var[M], dmu[d,M], dvar[d,M])."""
        Xs, M, ms, mg = self._lat_args(Xs, lat, mean_Xs, mean_grad)
        mu, var = np.zeros(M), np.zeros(M)
        dmu, dvar = np.zeros((self.d, M), order="F"), np.zeros((self.d, M), order="F")
        bad = C.c_long(-1)
        rc = load_library().boss_ngp_predict_grad_lat(self._h, M, _dp(Xs), lat._h, _dp(ms), _dp(mg), _dp(mu), _dp(var), _dp(dmu),
                                                      _dp(dvar), C.byref(bad))
        if rc == BOSS_E_NEG_VAR:
            e = DomainError(rc, load_library().boss_last_error().decode())
            e.bad_index = bad.value
            raise e
        _check(rc)
        return mu, var, dmu, dvar


LATENT_TARGETS = {"none": 0, "normal": 1, "lognormal": 2, "uniform": 3}       # BOSS_LT_*
LATENT_ACTS = {"identity": 0, "softplus": 1, "exp": 2}                          # BOSS_ACT_*


class NgpLatents:
    """The latent models of ONE output of a NonstationaryGP, resident on the device (boss_nlat_t): d lengthscale latents, the
    amplitude latent and optionally the noise latent.  Every latent is either a float (a constant, taken as it is) or a pair
    (gp, spec): `gp` a fitted plain GP handle, `spec` = (target, (p0, p1), activation, par) with the names of LATENT_TARGETS /
    LATENT_ACTS (or their codes).  create snapshots what the posterior means need: afterwards the handles may be updated or closed."""

    def __init__(self, lam, amp, noise=None, discrete=None, device: int = 0):
        lam = list(lam)
        d = len(lam)
        lats = lam + [amp, noise]
        nq = d + 2
        handles = (C.c_void_p * nq)()
        cst = np.full(nq, np.nan)
        tgt = (C.c_int * nq)()
        act = (C.c_int * nq)()
        tpar = np.zeros(2 * nq)
        apar = np.zeros(nq)
        for q, v in enumerate(lats):
            if v is None:
                if q != d + 1:
                    raise BossError(BOSS_E_INVALID, "only the noise latent may be left out")
                continue
            if isinstance(v, (tuple, list)):
                gp, (t, tp, a, ap) = v
                if getattr(gp, "_h", None) is None:             # a NULL handle would be read as "the constant beside it"
                    name = f"lengthscale latent {q}" if q < d else ("amplitude latent", "noise latent")[q - d]
                    raise BossError(BOSS_E_INVALID, f"the {name}'s GP handle is closed")
                handles[q] = gp._h
                tgt[q] = LATENT_TARGETS[t] if isinstance(t, str) else int(t)
                act[q] = LATENT_ACTS[a] if isinstance(a, str) else int(a)
                tpar[2 * q:2 * q + 2] = tp
                apar[q] = ap
            else:
                cst[q] = float(v)
        self.d = d
        self.device = device
        self.has_noise = noise is not None
        disc = None if discrete is None else np.ascontiguousarray(np.asarray(discrete, dtype=bool).astype(np.uint8))
        if disc is not None and disc.shape != (d,):
            raise BossError(BOSS_E_INVALID, "discrete must have one flag per dimension")
        h = C.c_void_p()
        self._h = None
        _check(load_library().boss_nlat_create(device, d, handles, _dp(cst), handles[d], float(cst[d]), handles[d + 1], float(cst[d + 1]),
                                               tgt, _dp(tpar), act, _dp(apar), _ucp(disc), C.byref(h)))
        self._h = h

    def eval(self, Xs, jac: bool = True, noise: bool = False):
        """λ(x*) d×M, α(x*) M[, σ(x*) M][, ∂λ/∂x d×d×M ([l, m, j] = ∂λ_l/∂x_m at candidate j), ∂α/∂x d×M] at the candidates
        (boss_nlat_eval): the arrays GibbsGP.predict / predict_grad take.  Returns (lam, amp, noise or None, dlam or None, damp or
        None).  An invalid value raises BossError (BOSS_E_INVALID) with .bad_index = the first such candidate."""
        Xs = _f64(Xs)
        if Xs.ndim == 1:
            Xs = _f64(Xs.reshape(-1, 1))
        if Xs.ndim != 2 or Xs.shape[0] != self.d:
            raise ValueError("candidates must be d×M")
        d, M = Xs.shape
        lam = np.zeros((d, M), order="F")
        amp = np.zeros(M)
        noi = np.zeros(M) if noise else None
        dl = np.zeros((d, d, M), order="F") if jac else None
        da = np.zeros((d, M), order="F") if jac else None
        bad = C.c_long(-1)
        rc = load_library().boss_nlat_eval(self._h, M, _dp(Xs), _dp(lam), _dp(amp), _dp(noi), _dp(dl), _dp(da), C.byref(bad))
        if rc != BOSS_OK:
            e = BossError(rc, load_library().boss_last_error().decode())
            e.bad_index = bad.value
            raise e
        return lam, amp, noi, dl, da

    def close(self):
        if self._h is not None:
            load_library().boss_nlat_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NgpWhitened:
    """One output slice of a NonstationaryGP with the whitening of its latent ParametrizedGPs resident on the device (boss_nfit_t):
    the data log-likelihood and its gradient w.r.t. the whitened parameters yϵ of S parameter sets in one call.
    factors: a sequence of N×N lower-triangular matrices (L of parametrized_gp.jl:200-202) or an N×N×F array; factor_of: d+2
    entries in latent order λ_0..λ_{d-1}, α, σ — an index into factors, or -1 for a scalar latent; specs: d+2 entries, for a GP
    latent (target, (p0, p1), activation, par) with the names of LATENT_TARGETS / LATENT_ACTS (or their codes), ignored (None) for
    scalar latents; mu: N×(d+2) or None.  Parameter layout: column s of theta (T×S) holds the latents in order, N values of yϵ per
    GP latent, one value (taken as it is) per scalar latent."""

    def __init__(self, X, y, factors, factor_of, specs, mu=None, mean_X=None, discrete=None, device: int = 0):
        X = _f64(X, 2)
        y = _f64(np.asarray(y).reshape(-1), 1)
        d, N = X.shape
        if y.shape[0] != N:
            raise ValueError("y must have one entry per column of X")
        nq = d + 2
        fo = np.ascontiguousarray(np.asarray(factor_of).reshape(-1), dtype=np.int32)
        specs = list(specs)
        if fo.shape[0] != nq or len(specs) != nq:
            raise BossError(BOSS_E_INVALID, "factor_of and specs must have d + 2 entries")
        if isinstance(factors, np.ndarray) and factors.ndim == 3:
            F = _f64(factors)
        else:
            fl = [_f64(f, 2) for f in factors]
            F = _f64(np.stack(fl, axis=2)) if fl else np.zeros((N, N, 0), order="F")
        if F.shape[:2] != (N, N):
            raise ValueError("every factor must be N×N")
        tgt = (C.c_int * nq)()
        act = (C.c_int * nq)()
        tpar = np.zeros(2 * nq)
        apar = np.zeros(nq)
        for q, sp in enumerate(specs):
            if sp is None or fo[q] < 0:
                continue
            t, tp, a, ap = sp
            tgt[q] = LATENT_TARGETS[t] if isinstance(t, str) else int(t)
            act[q] = LATENT_ACTS[a] if isinstance(a, str) else int(a)
            tpar[2 * q:2 * q + 2] = tp
            apar[q] = ap
        m = None if mu is None else _f64(mu, 2)
        if m is not None and m.shape != (N, nq):
            raise ValueError("mu must be N×(d+2)")
        mx = None if mean_X is None else _f64(np.asarray(mean_X).reshape(-1), 1)
        if mx is not None and mx.shape[0] != N:
            raise ValueError("mean_X must have N entries")
        disc = None if discrete is None else np.ascontiguousarray(np.asarray(discrete, dtype=bool).astype(np.uint8))
        if disc is not None and disc.shape != (d,):
            raise BossError(BOSS_E_INVALID, "discrete must have one flag per dimension")
        self.d, self.N, self.device = d, N, device
        self._h = None
        h = C.c_void_p()
        _check(load_library().boss_nfit_create(device, d, N, _dp(X), _dp(y), _ucp(disc), _dp(mx), F.shape[2], _dp(F),
                                               fo.ctypes.data_as(C.POINTER(C.c_int)), _dp(m), tgt, _dp(tpar), act, _dp(apar), C.byref(h)))
        self._h = h
        T = C.c_int(0)
        _check(load_library().boss_nfit_param_count(self._h, C.byref(T)))
        self.T = T.value

    def _theta(self, theta):
        th = _f64(theta)
        if th.ndim == 1:
            th = _f64(th.reshape(-1, 1))
        if th.ndim != 2 or th.shape[0] != self.T:
            raise ValueError(f"theta must be T×S with T = {self.T}")
        return th

    def values(self, theta):
        """(lam[d, N, S], amp[N, S], noise[N, S], status[S]): the latents' values at the data for every column of theta
        (boss_nfit_values), in the layouts ngp_loglike_batch takes."""
        th = self._theta(theta)
        S = th.shape[1]
        lam = np.zeros((self.d, self.N, S), order="F")
        amp, noi = np.zeros((self.N, S), order="F"), np.zeros((self.N, S), order="F")
        st = np.zeros(S, dtype=np.int32)
        _check(load_library().boss_nfit_values(self._h, S, _dp(th), _dp(lam), _dp(amp), _dp(noi), st.ctypes.data_as(C.POINTER(C.c_int))))
        return lam, amp, noi, st

    def loglike_grad(self, theta, want_grad: bool = True):
        """(ll[S], status[S], grad[T, S] or None): the data log-likelihood of every column of theta and its gradient w.r.t. theta
        (boss_nfit_loglike_grad); -Inf and a zero column where a set is invalid or not PD."""
        th = self._theta(theta)
        S = th.shape[1]
        ll = np.zeros(S)
        st = np.zeros(S, dtype=np.int32)
        grad = np.zeros((self.T, S), order="F") if want_grad else None
        _check(load_library().boss_nfit_loglike_grad(self._h, S, _dp(th), _dp(ll), _dp(grad), st.ctypes.data_as(C.POINTER(C.c_int))))
        return ll, st, grad

    def close(self):
        if self._h is not None:
            load_library().boss_nfit_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Candidates:
    """A resident batch of candidate points (boss_cand_t)."""

    def __init__(self, Xs, device: int = 0):
        Xs = _f64(Xs, 2)
        self.d, self.M = Xs.shape
        self.device = device
        h = C.c_void_p()
        _check(load_library().boss_cand_create(device, self.d, self.M, _dp(Xs), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            load_library().boss_cand_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fit(X, y, kernel, lengthscale, amplitude, noise_std, mean_X=None, discrete=None, device: int = 0,
        reserve: int = 0) -> GP:
    """posterior_gp (gaussian_process.jl:199-211) through the one-shot boss_gp_fit entry point.
    reserve > 0: room for that many later appends (create + reserve + update instead)."""
    if reserve > 0:
        g = GP(X, y, kernel, discrete, device)
        g.reserve(g.N + reserve)
        g.update(lengthscale, amplitude, noise_std, mean_X)
        return g
    lib = load_library()
    X = _f64(X, 2)
    y = _f64(np.asarray(y).reshape(-1), 1)
    lam = _f64(np.asarray(lengthscale).reshape(-1), 1)
    d, N = X.shape
    if lam.shape[0] != d:
        raise BossError(BOSS_E_INVALID, "length(lengthscales) must equal x_dim")
    m = None if mean_X is None else _f64(np.asarray(mean_X).reshape(-1), 1)
    disc = None if discrete is None else np.ascontiguousarray(np.asarray(discrete, dtype=bool).astype(np.uint8))
    h = C.c_void_p()
    out = C.c_double(0.0)
    _check(lib.boss_gp_fit(device, _kernel_id(kernel), d, N, _dp(X), _dp(y), _dp(m), _dp(lam), float(amplitude),
                           float(noise_std), _ucp(disc), C.byref(h), C.byref(out)))
    g = GP.__new__(GP)
    g.d, g.N, g.device, g.kernel, g._h, g.logpdf = d, N, device, _kernel_id(kernel), h, out.value
    return g


def fit_batch(X, y, kernel, lengthscales, amplitudes, noise_stds, mean_X=None, discrete=None, device: int = 0):
    """S resident posteriors of one output slice from ONE batched factorisation (boss_gp_fit_batch): what
    `model_posterior.(Ref(model), params, Ref(data))` builds for the S samples of a BI fit (src/posterior.jl:15-19).
    lengthscales is d×S.  Returns (gps[S], logpdf[S], status[S]); members with status != 0 are unfitted handles."""
    X = _f64(X, 2)
    y = _f64(np.asarray(y).reshape(-1), 1)
    lam = _f64(lengthscales, 2)
    d, N = X.shape
    S = lam.shape[1]
    if lam.shape[0] != d:
        raise BossError(BOSS_E_INVALID, "lengthscales must be d×S")
    amp = _f64(np.asarray(amplitudes).reshape(-1), 1)
    sig = _f64(np.asarray(noise_stds).reshape(-1), 1)
    if amp.shape[0] != S or sig.shape[0] != S:
        raise BossError(BOSS_E_INVALID, "amplitudes and noise_stds must have one entry per set")
    if y.shape[0] != N:
        raise ValueError("y must have one entry per column of X")           # (as GP.__init__: the library copies N entries)
    if not (np.isfinite(amp).all() and np.isfinite(sig).all() and np.isfinite(lam).all()):
        raise BossError(BOSS_E_INVALID, "hyper-parameters must be finite")
    stride = 0
    m = None
    if mean_X is not None:
        m = np.asarray(mean_X, dtype=np.float64)
        if m.ndim == 2:
            if m.shape != (S, N):
                raise ValueError("mean_X must be S×N (one prior-mean row per set) or a vector of N entries")
            m = np.ascontiguousarray(m)
            stride = N
        else:
            m = np.ascontiguousarray(m.reshape(-1))
            if m.shape[0] != N:
                raise ValueError("mean_X must be S×N (one prior-mean row per set) or a vector of N entries")
    disc = None if discrete is None else np.ascontiguousarray(np.asarray(discrete, dtype=bool).astype(np.uint8))
    hs = (C.c_void_p * S)()
    ll = np.zeros(S)
    st = np.zeros(S, dtype=np.int32)
    _check(load_library().boss_gp_fit_batch(device, _kernel_id(kernel), d, N, _dp(X), _dp(y), _dp(m), stride, _ucp(disc), S,
                                            _dp(lam), _dp(amp), _dp(sig), hs, _dp(ll), st.ctypes.data_as(C.POINTER(C.c_int))))
    gps = []
    for s in range(S):
        g = GP.__new__(GP)
        g.d, g.N, g.device, g.kernel, g._h = d, N, device, _kernel_id(kernel), C.c_void_p(hs[s])
        g.logpdf = float(ll[s]) if st[s] == 0 else None
        gps.append(g)
    return gps, ll, st


def loglike_batch(X, y, kernel, lengthscales, amplitudes, noise_stds, mean_X=None, discrete=None, device: int = 0,
                  want_grad: bool = False):
    """S log marginal likelihoods on the same (X, y) slice; lengthscales is d×S.
    Returns (ll[S], status[S]); ll = -Inf where the matrix is not PD (safe_data_loglike).
    want_grad: additionally grad[(d+2), S] = ∂ll/∂(lengthscale[d], amplitude, noise_std) per set -> (ll, status, grad)."""
    X = _f64(X, 2)
    y = _f64(np.asarray(y).reshape(-1), 1)
    lam = _f64(lengthscales, 2)
    d, N = X.shape
    S = lam.shape[1]
    if lam.shape[0] != d:
        raise BossError(BOSS_E_INVALID, "lengthscales must be d×S")
    amp = _f64(np.asarray(amplitudes).reshape(-1), 1)
    sig = _f64(np.asarray(noise_stds).reshape(-1), 1)
    stride = 0
    m = None
    if mean_X is not None:
        m = np.asarray(mean_X, dtype=np.float64)
        if m.ndim == 2:          # S×N, row s = mean of set s  → contiguous rows
            m = np.ascontiguousarray(m)
            stride = N
        else:
            m = np.ascontiguousarray(m.reshape(-1))
    disc = None if discrete is None else np.ascontiguousarray(np.asarray(discrete, dtype=bool).astype(np.uint8))
    ll = np.zeros(S)
    st = np.zeros(S, dtype=np.int32)
    if want_grad:
        grad = np.zeros((d + 2, S), order="F")
        _check(load_library().boss_gp_loglike_grad_batch(device, _kernel_id(kernel), d, N, _dp(X), _dp(y), _dp(m), stride,
                                                         _ucp(disc), S, _dp(lam), _dp(amp), _dp(sig), _dp(ll), _dp(grad),
                                                         st.ctypes.data_as(C.POINTER(C.c_int))))
        return ll, st, grad
    _check(load_library().boss_gp_loglike_batch(device, _kernel_id(kernel), d, N, _dp(X), _dp(y), _dp(m), stride,
                                                _ucp(disc), S, _dp(lam), _dp(amp), _dp(sig), _dp(ll),
                                                st.ctypes.data_as(C.POINTER(C.c_int))))
    return ll, st


def loglike_grad_batch_mean(X, y, kernel, lengthscales, amplitudes, noise_stds, mean_X=None, mean_jac=None, discrete=None,
                            device: int = 0, want_dmean: bool = False):
    """loglike_batch(..., want_grad=True) plus the gradient through the prior mean (boss_gp_loglike_grad_batch_mean).
    mean_X: None, N values shared by all sets, or S×N (row s = set s).  mean_jac: None, the Jacobian of the mean values w.r.t. T
    parameters of the mean as N×T (one matrix shared by all sets: a mean that is linear in them) or S×N×T (one per set).
    Returns (ll[S], status[S], grad[(d+2), S], dmean, dtheta): dmean N×S (column s = K⁻¹(y − m) of set s) if want_dmean else None,
    dtheta T×S (column s = mean_jac(s)ᵀ dmean(s), folded on the device) if mean_jac is given else None; zero columns where the
    status is not BOSS_OK."""
    X = _f64(X, 2)
    y = _f64(np.asarray(y).reshape(-1), 1)
    lam = _f64(lengthscales, 2)
    d, N = X.shape
    S = lam.shape[1]
    if lam.shape[0] != d:
        raise BossError(BOSS_E_INVALID, "lengthscales must be d×S")
    amp = _f64(np.asarray(amplitudes).reshape(-1), 1)
    sig = _f64(np.asarray(noise_stds).reshape(-1), 1)
    if y.shape[0] != N or amp.shape[0] != S or sig.shape[0] != S:
        raise ValueError("y must have N entries, amplitudes and noise_stds S each")
    stride = 0
    m = None
    if mean_X is not None:
        m = np.asarray(mean_X, dtype=np.float64)
        if m.ndim == 2:
            if m.shape != (S, N):
                raise ValueError("mean_X must be S×N (one prior-mean row per set) or a vector of N entries")
            m = np.ascontiguousarray(m)
            stride = N
        else:
            m = np.ascontiguousarray(m.reshape(-1))
            if m.shape[0] != N:
                raise ValueError("mean_X must be S×N (one prior-mean row per set) or a vector of N entries")
    T, jac, jac_stride = 0, None, 0
    if mean_jac is not None:
        jac = np.asarray(mean_jac, dtype=np.float64)
        if jac.ndim == 2 and jac.shape[0] == N and jac.shape[1] >= 1:
            T = jac.shape[1]
            jac = np.ascontiguousarray(jac.T)                  # N×T column-major
        elif jac.ndim == 3 and jac.shape[:2] == (S, N) and jac.shape[2] >= 1:
            T = jac.shape[2]
            jac = np.ascontiguousarray(jac.transpose(0, 2, 1))  # set after set, each N×T column-major
            jac_stride = N * T
        else:
            raise ValueError("mean_jac must be N×T (shared by all sets) or S×N×T, T >= 1")
    disc = None if discrete is None else np.ascontiguousarray(np.asarray(discrete, dtype=bool).astype(np.uint8))
    ll = np.zeros(S)
    st = np.zeros(S, dtype=np.int32)
    grad = np.zeros((d + 2, S), order="F")
    dmean = np.zeros((N, S), order="F") if want_dmean else None
    dtheta = np.zeros((T, S), order="F") if T else None
    _check(load_library().boss_gp_loglike_grad_batch_mean(device, _kernel_id(kernel), d, N, _dp(X), _dp(y), _dp(m), stride, _ucp(disc), S,
                                                          _dp(lam), _dp(amp), _dp(sig), T, _dp(jac), jac_stride, _dp(ll), _dp(grad),
                                                          _dp(dmean), _dp(dtheta), st.ctypes.data_as(C.POINTER(C.c_int))))
    return ll, st, grad, dmean, dtheta


def _ggp_batch_args(X, y, dY, lengthscales, amplitudes, noise_stds, grad_noise_stds):
    """The arrays boss_ggp_loglike_batch reads, converted and checked (no device is touched): X d×n, y n, dY d×n, lengthscales d×S,
    the other parameters S each — all float64, matrices column-major."""
    X = _f64(X, 2)
    d, n = X.shape
    y = _f64(np.asarray(y).reshape(-1), 1)
    dY = _f64(dY, 2)
    if y.shape[0] != n or dY.shape != (d, n):
        raise ValueError("y must have n entries and dY must be d×n")
    lam = _f64(lengthscales, 2)
    if lam.shape[0] != d:
        raise BossError(BOSS_E_INVALID, "lengthscales must be d×S")
    S = lam.shape[1]
    amp, sig, sgd = (_f64(np.asarray(a).reshape(-1), 1) for a in (amplitudes, noise_stds, grad_noise_stds))
    if amp.shape[0] != S or sig.shape[0] != S or sgd.shape[0] != S:
        raise BossError(BOSS_E_INVALID, "amplitudes, noise_stds and grad_noise_stds must have one entry per column of lengthscales")
    return X, y, dY, lam, amp, sig, sgd


def ggp_loglike_batch(X, y, dY, kernel, lengthscales, amplitudes, noise_stds, grad_noise_stds, device: int = 0):
    """S log marginal likelihoods of the gradient-observation model on one (X, y, dY) slice in one device call
    (boss_ggp_loglike_batch); lengthscales is d×S.  Returns (ll[S], status[S]); ll = -Inf where the augmented matrix is not PD
    or a parameter is negative."""
    X, y, dY, lam, amp, sig, sgd = _ggp_batch_args(X, y, dY, lengthscales, amplitudes, noise_stds, grad_noise_stds)
    d, n = X.shape
    S = lam.shape[1]
    ll = np.zeros(S)
    st = np.zeros(S, dtype=np.int32)
    _check(load_library().boss_ggp_loglike_batch(device, _kernel_id(kernel), d, n, _dp(X), _dp(y), _dp(dY), S, _dp(lam), _dp(amp),
                                                 _dp(sig), _dp(sgd), _dp(ll), st.ctypes.data_as(C.POINTER(C.c_int))))
    return ll, st


def _ngp_batch_args(X, y, lam_X, amp_X, noise_X, mean_X=None, discrete=None):
    """The arrays boss_ngp_loglike_batch reads, converted and checked (no device is touched): X d×N, y N, lam_X d×N×S, amp_X and
    noise_X N×S (column s = set s), mean_X None, N values shared by the sets, or S×N (row s = set s).  Returns them with the
    mean stride (0 or N) and the uint8 discrete flags."""
    X = _f64(X, 2)
    d, N = X.shape
    y = _f64(np.asarray(y).reshape(-1), 1)
    if y.shape[0] != N:
        raise ValueError("y must have one entry per column of X")
    lam = _f64(lam_X, 3)
    if lam.shape[:2] != (d, N):
        raise BossError(BOSS_E_INVALID, "lam_X must be d×N×S")
    S = lam.shape[2]
    amp = _f64(amp_X, 2)
    noi = _f64(noise_X, 2)
    if amp.shape != (N, S) or noi.shape != (N, S):
        raise BossError(BOSS_E_INVALID, "amp_X and noise_X must be N×S")
    stride = 0
    m = None
    if mean_X is not None:
        m = np.asarray(mean_X, dtype=np.float64)
        if m.ndim == 2:          # S×N, row s = mean of set s  → contiguous rows
            if m.shape != (S, N):
                raise BossError(BOSS_E_INVALID, "a per-set mean_X must be S×N")
            m = np.ascontiguousarray(m)
            stride = N
        else:
            m = np.ascontiguousarray(m.reshape(-1))
            if m.shape[0] != N:
                raise BossError(BOSS_E_INVALID, "a shared mean_X must have N entries")
    disc = None if discrete is None else np.ascontiguousarray(np.asarray(discrete, dtype=bool).astype(np.uint8))
    if disc is not None and disc.shape != (d,):
        raise BossError(BOSS_E_INVALID, "discrete must have one flag per dimension")
    return X, y, lam, amp, noi, m, stride, disc


def ngp_loglike_batch(X, y, lam_X, amp_X, noise_X, mean_X=None, discrete=None, device: int = 0):
    """S log marginal likelihoods of the nonstationary model on one (X, y) slice in one device call (boss_ngp_loglike_batch): the
    latent models' values at the (rounded) data for every set, lam_X d×N×S, amp_X N×S, noise_X N×S.  Returns (ll[S], status[S]);
    ll = -Inf where the matrix is not PD or a latent value is negative, NaN or infinite."""
    X, y, lam, amp, noi, m, stride, disc = _ngp_batch_args(X, y, lam_X, amp_X, noise_X, mean_X, discrete)
    d, N = X.shape
    S = lam.shape[2]
    ll = np.zeros(S)
    st = np.zeros(S, dtype=np.int32)
    _check(load_library().boss_ngp_loglike_batch(device, d, N, _dp(X), _dp(y), _ucp(disc), S, _dp(lam), _dp(amp), _dp(noi), _dp(m),
                                                 stride, _dp(ll), st.ctypes.data_as(C.POINTER(C.c_int))))
    return ll, st


def ggp_loglike_grad_batch(X, y, dY, kernel, lengthscales, amplitudes, noise_stds, grad_noise_stds, device: int = 0):
    """ggp_loglike_batch with the gradient of every log-likelihood in the same device call (boss_ggp_loglike_grad_batch): what
    GradGP.update + GradGP.loglike_grad give set by set.  Returns (ll[S], status[S], grad[(d+3), S]); column s of grad is
    ∂ℓ/∂(λ_1..λ_d, α, σ, σ_∂) of set s, zeros (and ll = -Inf) where the set is not PD or holds a negative parameter."""
    X, y, dY, lam, amp, sig, sgd = _ggp_batch_args(X, y, dY, lengthscales, amplitudes, noise_stds, grad_noise_stds)
    d, n = X.shape
    S = lam.shape[1]
    ll = np.zeros(S)
    st = np.zeros(S, dtype=np.int32)
    grad = np.zeros((d + 3, S), order="F")
    _check(load_library().boss_ggp_loglike_grad_batch(device, _kernel_id(kernel), d, n, _dp(X), _dp(y), _dp(dY), S, _dp(lam),
                                                      _dp(amp), _dp(sig), _dp(sgd), _dp(ll), _dp(grad),
                                                      st.ctypes.data_as(C.POINTER(C.c_int))))
    return ll, st, grad


def ngp_loglike_grad_batch(X, y, lam_X, amp_X, noise_X, mean_X=None, discrete=None, device: int = 0):
    """ngp_loglike_batch with the partial derivatives w.r.t. the latent values of every set in the same device call
    (boss_ngp_loglike_grad_batch): what NonstatGP.update + NonstatGP.loglike_grad give set by set.  Returns (ll[S], status[S],
    dlam[d, N, S], damp[N, S], dnoise[N, S], dmean[N, S]); zeros (and ll = -Inf) where a set is not PD or invalid."""
    X, y, lam, amp, noi, m, stride, disc = _ngp_batch_args(X, y, lam_X, amp_X, noise_X, mean_X, discrete)
    d, N = X.shape
    if d > 16:
        raise BossError(BOSS_E_INVALID, "x_dim above 16 is not supported by the nonstationary gradient kernels")
    S = lam.shape[2]
    ll = np.zeros(S)
    st = np.zeros(S, dtype=np.int32)
    dlam = np.zeros((d, N, S), order="F")
    damp, dnoise, dmean = (np.zeros((N, S), order="F") for _ in range(3))
    _check(load_library().boss_ngp_loglike_grad_batch(device, d, N, _dp(X), _dp(y), _ucp(disc), S, _dp(lam), _dp(amp), _dp(noi),
                                                      _dp(m), stride, _dp(ll), _dp(dlam), _dp(damp), _dp(dnoise), _dp(dmean),
                                                      st.ctypes.data_as(C.POINTER(C.c_int))))
    return ll, st, dlam, damp, dnoise, dmean


def ggp_fit_batch(X, y, dY, kernel, lengthscales, amplitudes, noise_stds, grad_noise_stds, device: int = 0):
    """S resident posteriors of the gradient-observation model on one (X, y, dY) slice from ONE batched factorisation
    (boss_ggp_fit_batch): what model_posterior builds per sample of a BI fit (src/posterior.jl:15-19).  Arguments as
    ggp_loglike_batch.  Returns (gps[S] of GradGP, logpdf[S], status[S]); members with status != 0 are unfitted handles."""
    X, y, dY, lam, amp, sig, sgd = _ggp_batch_args(X, y, dY, lengthscales, amplitudes, noise_stds, grad_noise_stds)
    d, n = X.shape
    S = lam.shape[1]
    if S < 1:
        raise BossError(BOSS_E_INVALID, "at least one parameter set is needed")
    hs = (C.c_void_p * S)()
    ll = np.zeros(S)
    st = np.zeros(S, dtype=np.int32)
    _check(load_library().boss_ggp_fit_batch(device, _kernel_id(kernel), d, n, _dp(X), _dp(y), _dp(dY), S, _dp(lam), _dp(amp),
                                             _dp(sig), _dp(sgd), hs, _dp(ll), st.ctypes.data_as(C.POINTER(C.c_int))))
    gps = []
    for s in range(S):
        g = GradGP.__new__(GradGP)
        g.d, g.n, g.N, g.device, g.kernel, g._h = d, n, n * (1 + d), device, _kernel_id(kernel), C.c_void_p(hs[s])
        g.logpdf = float(ll[s]) if st[s] == 0 else None
        gps.append(g)
    return gps, ll, st


def ngp_fit_batch(X, y, lam_X, amp_X, noise_X, mean_X=None, discrete=None, device: int = 0):
    """S resident posteriors of the nonstationary model on one (X, y) slice from ONE batched factorisation (boss_ngp_fit_batch).
    Arguments as ngp_loglike_batch.  Returns (gps[S] of GibbsGP, logpdf[S], status[S]); members with status != 0 are unfitted."""
    X, y, lam, amp, noi, m, stride, disc = _ngp_batch_args(X, y, lam_X, amp_X, noise_X, mean_X, discrete)
    d, N = X.shape
    S = lam.shape[2]
    if S < 1:
        raise BossError(BOSS_E_INVALID, "at least one parameter set is needed")
    hs = (C.c_void_p * S)()
    ll = np.zeros(S)
    st = np.zeros(S, dtype=np.int32)
    _check(load_library().boss_ngp_fit_batch(device, d, N, _dp(X), _dp(y), _ucp(disc), S, _dp(lam), _dp(amp), _dp(noi), _dp(m),
                                             stride, hs, _dp(ll), st.ctypes.data_as(C.POINTER(C.c_int))))
    gps = []
    for s in range(S):
        g = GibbsGP.__new__(GibbsGP)
        g.d, g.N, g.device, g.kernel, g._h = d, N, device, None, C.c_void_p(hs[s])
        g.logpdf = float(ll[s]) if st[s] == 0 else None
        gps.append(g)
    return gps, ll, st


def _ngp_set_args(n, d, Xs, lam_Xs, amp_Xs, mean_Xs):
    """The arrays boss_ngp_predict_set reads, converted and checked (no device is touched): Xs d×M, lam_Xs d×M×n, amp_Xs M×n (column i =
    member i), mean_Xs None or n×M (row i = member i)."""
    Xs = _f64(Xs)
    if Xs.ndim == 1:
        Xs = _f64(Xs.reshape(-1, 1))
    if Xs.ndim != 2 or Xs.shape[0] != d:
        raise ValueError("candidates must be d×M")
    M = Xs.shape[1]
    lam = _f64(lam_Xs, 3)
    amp = _f64(amp_Xs, 2)
    if lam.shape != (d, M, n) or amp.shape != (M, n):
        raise BossError(BOSS_E_INVALID, "lam_Xs must be d×M×n and amp_Xs M×n (n = number of posteriors)")
    ms = None
    if mean_Xs is not None:
        ms = np.ascontiguousarray(np.asarray(mean_Xs, dtype=np.float64))
        if ms.shape != (n, M):
            raise BossError(BOSS_E_INVALID, "mean_Xs must be n×M (one row per posterior)")
    return Xs, lam, amp, ms


def ngp_predict_set(gps: Sequence["GibbsGP"], Xs, lam_Xs, amp_Xs, mean_Xs=None):
    """mean_and_var of n nonstationary posteriors at the same candidates in one call (boss_ngp_predict_set): lam_Xs d×M×n and
    amp_Xs M×n are every member's λ(x*), α(x*).  Returns (mu[n, M], var[n, M]) — what acq_ei_moments takes as mu[S][1][M].
    Equally shaped handles (the members of an ngp_fit_batch) are predicted in one launch.  DomainError (with .bad_index) as
    GibbsGP.predict."""
    n = len(gps)
    if n < 1:
        raise BossError(BOSS_E_INVALID, "at least one posterior is needed")
    d = gps[0].d
    Xs, lam, amp, ms = _ngp_set_args(n, d, Xs, lam_Xs, amp_Xs, mean_Xs)
    M = Xs.shape[1]
    arr = (C.c_void_p * n)(*[g._h.value for g in gps])
    mu = np.zeros((n, M))
    var = np.zeros((n, M))
    bad = C.c_long(-1)
    rc = load_library().boss_ngp_predict_set(n, arr, M, _dp(Xs), _dp(lam), _dp(amp), _dp(ms), _dp(mu), _dp(var), C.byref(bad))
    if rc == BOSS_E_NEG_VAR:
        e = DomainError(rc, load_library().boss_last_error().decode())
        e.bad_index = bad.value
        raise e
    _check(rc)
    return mu, var


def _lat_set_args(gps, lats, Xs, mean_Xs, mean_grad=None):
    """What the _lat set calls read, converted and checked (no device is touched)."""
    n = len(gps)
    if n < 1 or len(lats) != n:
        raise BossError(BOSS_E_INVALID, "one latent object per posterior is needed (at least one)")
    if any(not isinstance(L, NgpLatents) or L._h is None for L in lats):
        raise BossError(BOSS_E_INVALID, "lats must be open NgpLatents")
    d = gps[0].d
    Xs = _f64(Xs)
    if Xs.ndim == 1:
        Xs = _f64(Xs.reshape(-1, 1))
    if Xs.ndim != 2 or Xs.shape[0] != d:
        raise ValueError("candidates must be d×M")
    M = Xs.shape[1]
    ms = mg = None
    if mean_Xs is not None:
        ms = np.ascontiguousarray(np.asarray(mean_Xs, dtype=np.float64))
        if ms.shape != (n, M):
            raise BossError(BOSS_E_INVALID, "mean_Xs must be n×M (one row per posterior)")
    if mean_grad is not None:
        a = np.asarray(mean_grad, dtype=np.float64)
        if a.shape != (n, d, M):
            raise BossError(BOSS_E_INVALID, "mean_grad must be n×d×M (one block per posterior)")
        mg = np.ascontiguousarray(a.transpose(0, 2, 1))
    arr = (C.c_void_p * n)(*[g._h.value for g in gps])
    larr = (C.c_void_p * n)(*[L._h.value for L in lats])
    return n, d, M, Xs, ms, mg, arr, larr


def ngp_predict_set_lat(gps: Sequence["GibbsGP"], Xs, lats: Sequence["NgpLatents"], mean_Xs=None):
    """ngp_predict_set with every member's λ(x*), α(x*) read from its resident latent models (boss_ngp_predict_set_lat)."""
    gps, lats = list(gps), list(lats)
    n, d, M, Xs, ms, _, arr, larr = _lat_set_args(gps, lats, Xs, mean_Xs)
    mu, var = np.zeros((n, M)), np.zeros((n, M))
    bad = C.c_long(-1)
    rc = load_library().boss_ngp_predict_set_lat(n, arr, M, _dp(Xs), larr, _dp(ms), _dp(mu), _dp(var), C.byref(bad))
    if rc == BOSS_E_NEG_VAR:
        e = DomainError(rc, load_library().boss_last_error().decode())
        e.bad_index = bad.value
        raise e
    _check(rc)
    return mu, var


def ngp_predict_grad_set_lat(gps: Sequence["GibbsGP"], Xs, lats: Sequence["NgpLatents"], mean_Xs=None, mean_grad=None):
    """ngp_predict_grad_set with every member's latent values and analytic Jacobians read from its resident latent models
    (boss_ngp_predict_grad_set_lat).  Returns (mu[n, M], var[n, M], dmu[n, d, M], dvar[n, d, M])."""
    gps, lats = list(gps), list(lats)
    n, d, M, Xs, ms, mg, arr, larr = _lat_set_args(gps, lats, Xs, mean_Xs, mean_grad)
    mu, var = np.zeros((n, M)), np.zeros((n, M))
    dmu, dvar = np.zeros((n, M, d)), np.zeros((n, M, d))
    bad = C.c_long(-1)
    rc = load_library().boss_ngp_predict_grad_set_lat(n, arr, M, _dp(Xs), larr, _dp(ms), _dp(mg), _dp(mu), _dp(var), _dp(dmu), _dp(dvar),
                                                      C.byref(bad))
    if rc == BOSS_E_NEG_VAR:
        e = DomainError(rc, load_library().boss_last_error().decode())
        e.bad_index = bad.value
        raise e
    _check(rc)
    return mu, var, dmu.transpose(0, 2, 1), dvar.transpose(0, 2, 1)


def ngp_acq_ei_grad_set_lat(gps: Sequence[Sequence["GibbsGP"]], Xs, lats: Sequence[Sequence["NgpLatents"]], fit_coefs, y_max=None,
                            best=None, valid_mask=None, mean_Xs=None, mean_grad=None):
    """ngp_acq_ei_grad_set with the latent values and Jacobians of member gps[s][p] read from lats[s][p] on the device
    (boss_ngp_acq_ei_grad_set_lat).  Returns (acq[M], dacq[d, M])."""
    S = len(gps)
    P = len(gps[0]) if S else 0
    if S < 1 or P < 1 or any(len(row) != P for row in gps) or len(lats) != S or any(len(row) != P for row in lats):
        raise BossError(BOSS_E_INVALID, "gps and lats must be S rows of P")
    flat_g = [gps[s][p] for s in range(S) for p in range(P)]                 # member i = p + P·s
    flat_l = [lats[s][p] for s in range(S) for p in range(P)]
    n, d, M, Xs, ms, mg, arr, larr = _lat_set_args(flat_g, flat_l, Xs, mean_Xs, mean_grad)
    coefs = _f64(np.asarray(fit_coefs).reshape(-1), 1)
    if coefs.shape[0] != P:
        raise BossError(BOSS_E_INVALID, "fit_coefs must have one entry per output")
    ym = None if y_max is None else _f64(np.asarray(y_max).reshape(-1), 1)
    if ym is not None and ym.shape[0] != P:
        raise BossError(BOSS_E_INVALID, "y_max must have one entry per output")
    mask = None if valid_mask is None else np.ascontiguousarray(np.asarray(valid_mask, dtype=bool).astype(np.uint8))
    if mask is not None and mask.shape != (M,):
        raise BossError(BOSS_E_INVALID, "valid_mask must have one entry per candidate")
    acq = np.zeros(M)
    dacq = np.zeros((d, M), order="F")
    _check(load_library().boss_ngp_acq_ei_grad_set_lat(P, S, arr, M, _dp(Xs), larr, _dp(ms), _dp(mg), _dp(coefs), _dp(ym),
                                                       0 if best is None else 1, 0.0 if best is None else float(best), _ucp(mask),
                                                       _dp(acq), _dp(dacq)))
    return acq, dacq


def acq_ei(gps: Sequence[Sequence[GP]], cand: Candidates, fit_coefs, y_max=None, best=None, valid_mask=None,
           mean_Xs=None, want_acq: bool = True):
    """EI·feas over resident candidates.  gps[s][p] = output p of hyper-parameter sample s.
    mean_Xs: None or array [S][P][M].  Returns (acq[M] or None, argmax, max)."""
    S = len(gps)
    P = len(gps[0])
    arr = (C.c_void_p * (P * S))()
    for s in range(S):
        for p in range(P):
            arr[p + P * s] = gps[s][p]._h
    coefs = _f64(np.asarray(fit_coefs).reshape(-1), 1)
    ym = None if y_max is None else _f64(np.asarray(y_max).reshape(-1), 1)
    mask = None if valid_mask is None else np.ascontiguousarray(np.asarray(valid_mask, dtype=bool).astype(np.uint8))
    M = cand.M
    ms = None
    if mean_Xs is not None:
        a = np.asarray(mean_Xs, dtype=np.float64).reshape(S, P, M)
        ms = np.ascontiguousarray(a.transpose(0, 2, 1))       # index p + P*(j + M*s)
    acq = np.zeros(M) if want_acq else None
    am = C.c_long(-1)
    mx = C.c_double(0.0)
    _check(load_library().boss_acq_ei(P, S, arr, cand._h, _dp(ms), _dp(coefs), _dp(ym), 0 if best is None else 1,
                                      0.0 if best is None else float(best), _ucp(mask), _dp(acq), C.byref(am),
                                      C.byref(mx)))
    return acq, am.value, mx.value


def acq_ei_grad_moments(mu, var, dmu, dvar, fit_coefs, y_max=None, best=None, valid_mask=None, device: int = 0):
    """EI × feasibility and its gradient w.r.t. the candidates from moments and moment gradients already on the host
    (boss_acq_ei_grad_moments): mu / var [P][M], dmu / dvar [P][d][M].  Returns (acq[M], dacq[d, M])."""
    mu = np.ascontiguousarray(np.atleast_2d(np.asarray(mu, dtype=np.float64)))       # row p at p*M
    var = np.ascontiguousarray(np.atleast_2d(np.asarray(var, dtype=np.float64)))
    if mu.ndim != 2 or var.shape != mu.shape:
        raise ValueError("mu and var must both be P×M")
    P, M = mu.shape
    gm = np.asarray(dmu, dtype=np.float64).reshape(P, -1, M)
    gv = np.asarray(dvar, dtype=np.float64).reshape(P, -1, M)
    d = gm.shape[1]
    gm = np.ascontiguousarray(gm.transpose(0, 2, 1))          # [p][j*d + m]
    gv = np.ascontiguousarray(gv.transpose(0, 2, 1))
    coefs = _f64(np.asarray(fit_coefs).reshape(-1), 1)
    ym = None if y_max is None else _f64(np.asarray(y_max).reshape(-1), 1)
    mask = None if valid_mask is None else np.ascontiguousarray(np.asarray(valid_mask, dtype=bool).astype(np.uint8))
    acq = np.zeros(M)
    dacq = np.zeros((d, M), order="F")
    _check(load_library().boss_acq_ei_grad_moments(device, P, M, d, _dp(mu), _dp(var), _dp(gm), _dp(gv), _dp(coefs), _dp(ym),
                                                   0 if best is None else 1, 0.0 if best is None else float(best), _ucp(mask), _dp(acq),
                                                   _dp(dacq)))
    return acq, dacq


class Track:
    """Resident predictive state of one posterior at one candidate set (boss_track_t): after
    GP.append the moments are extended in O(N·M) instead of re-solved.  Keep `gp` and `cand` alive."""

    def __init__(self, gp: GP, cand: Candidates, mean_Xs=None):
        ms = None if mean_Xs is None else _f64(np.asarray(mean_Xs).reshape(-1), 1)
        if ms is not None and ms.shape[0] != cand.M:
            raise ValueError("mean_Xs must have one entry per candidate")
        h = C.c_void_p()
        _check(load_library().boss_track_create(gp._h, cand._h, _dp(ms), C.byref(h)))
        self._h, self.gp, self.cand, self.M = h, gp, cand, cand.M

    def sync(self):
        _check(load_library().boss_track_sync(self._h))

    def moments(self, first: int = 0, count: Optional[int] = None):
        """(mu, var) of candidates [first, first+count) — var unclipped (apply _clip_var yourself)."""
        count = self.M - first if count is None else count
        mu, var = np.zeros(count), np.zeros(count)
        _check(load_library().boss_track_moments(self._h, first, count, _dp(mu), _dp(var)))
        return mu, var

    def close(self):
        if getattr(self, "_h", None):
            load_library().boss_track_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GibbsTrack(Track):
    """Track of a nonstationary posterior (boss_ngp_track_create[_lat]): extended in O(N·M) after GibbsGP.append.  Exactly one of
    the arrays (lam_Xs d×M and amp_Xs M: λ(x*), α(x*) at the candidates, rounded where dims are discrete) and `latents` (an
    NgpLatents, evaluated on the device) is given.  Has Track's methods and goes to acq_ei_tracks like one."""

    def __init__(self, gp: "GibbsGP", cand: Candidates, lam_Xs=None, amp_Xs=None, mean_Xs=None, latents: Optional[NgpLatents] = None):
        arrays = lam_Xs is not None or amp_Xs is not None
        if arrays == (latents is not None):
            raise ValueError("give either lam_Xs and amp_Xs or latents")
        if arrays and (lam_Xs is None or amp_Xs is None):
            raise ValueError("lam_Xs and amp_Xs go together")
        d, M = cand.d, cand.M
        ms = None if mean_Xs is None else _f64(np.asarray(mean_Xs).reshape(-1), 1)
        if ms is not None and ms.shape[0] != M:
            raise ValueError("mean_Xs must have one entry per candidate")
        h = C.c_void_p()
        if arrays:
            lam = _f64(lam_Xs)
            amp = _f64(np.asarray(amp_Xs).reshape(-1), 1)
            if lam.shape != (d, M) or amp.shape[0] != M:
                raise ValueError("lam_Xs must be d×M and amp_Xs length M")
            _check(load_library().boss_ngp_track_create(gp._h, cand._h, _dp(lam), _dp(amp), _dp(ms), C.byref(h)))
        else:
            if not isinstance(latents, NgpLatents):
                raise ValueError("latents must be an NgpLatents")
            if latents._h is None:
                raise BossError(BOSS_E_INVALID, "latents must be an open NgpLatents")
            _check(load_library().boss_ngp_track_create_lat(gp._h, cand._h, latents._h, _dp(ms), C.byref(h)))
        self._h, self.gp, self.cand, self.M = h, gp, cand, M


class GradTrack(Track):
    """Track of a gradient-observation posterior (boss_ggp_track_create): extended in O(N·M) per appended row after
    GradGP.append.  Has Track's methods and goes to acq_ei_tracks like one; `moments` returns the reference's max(0, σ²)."""

    def __init__(self, gp: "GradGP", cand: Candidates):
        h = C.c_void_p()
        _check(load_library().boss_ggp_track_create(gp._h, cand._h, C.byref(h)))
        self._h, self.gp, self.cand, self.M = h, gp, cand, cand.M


def acq_ei_tracks(tracks: Sequence[Sequence[Track]], fit_coefs, y_max=None, best=None, valid_mask=None,
                  want_acq: bool = True):
    """acq_ei on tracked states: tracks[s][p] = output p of hyper-parameter sample s."""
    S, P = len(tracks), len(tracks[0])
    arr = (C.c_void_p * (P * S))()
    for s in range(S):
        for p in range(P):
            arr[p + P * s] = tracks[s][p]._h
    M = tracks[0][0].M
    coefs = _f64(np.asarray(fit_coefs).reshape(-1), 1)
    ym = None if y_max is None else _f64(np.asarray(y_max).reshape(-1), 1)
    mask = None if valid_mask is None else np.ascontiguousarray(np.asarray(valid_mask, dtype=bool).astype(np.uint8))
    acq = np.zeros(M) if want_acq else None
    am = C.c_long(-1)
    mx = C.c_double(0.0)
    _check(load_library().boss_acq_ei_tracks(P, S, arr, _dp(coefs), _dp(ym), 0 if best is None else 1,
                                             0.0 if best is None else float(best), _ucp(mask), _dp(acq), C.byref(am),
                                             C.byref(mx)))
    return acq, am.value, mx.value


def acq_ei_grad(gps: Sequence[GP], Xs, fit_coefs, y_max=None, best=None, valid_mask=None, mean_Xs=None, mean_grad=None):
    """EI·feas and its gradient w.r.t. the candidates for one hyper-parameter sample.  gps[p] = output p.
    mean_Xs: None or [P][M]; mean_grad: None or [P][d][M].  Returns (acq[M], dacq[d, M])."""
    P = len(gps)
    Xs = _f64(Xs, 2)
    d, M = Xs.shape
    arr = (C.c_void_p * P)()
    for p in range(P):
        arr[p] = gps[p]._h
    coefs = _f64(np.asarray(fit_coefs).reshape(-1), 1)
    ym = None if y_max is None else _f64(np.asarray(y_max).reshape(-1), 1)
    mask = None if valid_mask is None else np.ascontiguousarray(np.asarray(valid_mask, dtype=bool).astype(np.uint8))
    ms = None if mean_Xs is None else np.ascontiguousarray(np.asarray(mean_Xs, dtype=np.float64).reshape(P, M))
    mg = None
    if mean_grad is not None:
        a = np.asarray(mean_grad, dtype=np.float64).reshape(P, d, M)
        mg = np.ascontiguousarray(a.transpose(0, 2, 1))           # [p][j*d + m]
    acq = np.zeros(M)
    dacq = np.zeros((d, M), order="F")
    _check(load_library().boss_acq_ei_grad(P, arr, M, _dp(Xs), _dp(ms), _dp(mg), _dp(coefs), _dp(ym),
                                           0 if best is None else 1, 0.0 if best is None else float(best), _ucp(mask),
                                           _dp(acq), _dp(dacq)))
    return acq, dacq


def acq_ei_grad_set(gps: Sequence[Sequence[GP]], Xs, fit_coefs, y_max=None, best=None, valid_mask=None, mean_Xs=None, mean_grad=None):
    """EI·feas and its gradient w.r.t. the candidates, averaged over S hyper-parameter samples in ONE device call
    (boss_acq_ei_grad_set).  gps[s][p] = output p of sample s.  mean_Xs: None or [S][P][M]; mean_grad: None or [S][P][d][M].
    Returns (acq[M], dacq[d, M]) = the means over s of what acq_ei_grad returns for gps[s]."""
    S = len(gps)
    P = len(gps[0]) if S else 0
    if S < 1 or P < 1 or any(len(row) != P for row in gps):
        raise BossError(BOSS_E_INVALID, "gps must be S rows of P posteriors")
    Xs = _f64(Xs, 2)
    d, M = Xs.shape
    arr = (C.c_void_p * (P * S))()
    for s in range(S):
        for p in range(P):
            arr[p + P * s] = gps[s][p]._h
    coefs = _f64(np.asarray(fit_coefs).reshape(-1), 1)
    ym = None if y_max is None else _f64(np.asarray(y_max).reshape(-1), 1)
    mask = None if valid_mask is None else np.ascontiguousarray(np.asarray(valid_mask, dtype=bool).astype(np.uint8))
    ms = None if mean_Xs is None else np.ascontiguousarray(np.asarray(mean_Xs, dtype=np.float64).reshape(S, P, M))
    mg = None
    if mean_grad is not None:
        a = np.asarray(mean_grad, dtype=np.float64).reshape(S, P, d, M)
        mg = np.ascontiguousarray(a.transpose(0, 1, 3, 2))        # [s][p][j*d + m]
    acq = np.zeros(M)
    dacq = np.zeros((d, M), order="F")
    _check(load_library().boss_acq_ei_grad_set(P, S, arr, M, _dp(Xs), _dp(ms), _dp(mg), _dp(coefs), _dp(ym),
                                               0 if best is None else 1, 0.0 if best is None else float(best), _ucp(mask),
                                               _dp(acq), _dp(dacq)))
    return acq, dacq


def _ngp_grad_set_args(n, d, Xs, lam_Xs, amp_Xs, dlam_Xs, damp_Xs, mean_Xs, mean_grad):
    """The arrays boss_ngp_predict_grad_set / boss_ngp_acq_ei_grad_set read beside those of _ngp_set_args, converted and checked (no
    device is touched): dlam_Xs None or d×d×M×n ([l, m, j, i] = ∂λ_l/∂x_m of member i at candidate j), damp_Xs None or d×M×n,
    mean_Xs None or n×M, mean_grad None or n×d×M (-> [i][j*d + m])."""
    Xs, lam, amp, ms = _ngp_set_args(n, d, Xs, lam_Xs, amp_Xs, mean_Xs)
    M = Xs.shape[1]
    dl = da = mg = None
    if dlam_Xs is not None:
        dl = _f64(dlam_Xs, 4)
        if dl.shape != (d, d, M, n):
            raise BossError(BOSS_E_INVALID, "dlam_Xs must be d×d×M×n")
    if damp_Xs is not None:
        da = _f64(damp_Xs, 3)
        if da.shape != (d, M, n):
            raise BossError(BOSS_E_INVALID, "damp_Xs must be d×M×n")
    if mean_grad is not None:
        a = np.asarray(mean_grad, dtype=np.float64)
        if a.shape != (n, d, M):
            raise BossError(BOSS_E_INVALID, "mean_grad must be n×d×M (one block per posterior)")
        mg = np.ascontiguousarray(a.transpose(0, 2, 1))
    return Xs, lam, amp, dl, da, ms, mg


def ngp_predict_grad_set(gps: Sequence["GibbsGP"], Xs, lam_Xs, amp_Xs, dlam_Xs=None, damp_Xs=None, mean_Xs=None, mean_grad=None):
    """GibbsGP.predict_grad of n nonstationary posteriors at the same candidates in one call (boss_ngp_predict_grad_set): lam_Xs
    d×M×n, amp_Xs M×n, dlam_Xs d×d×M×n, damp_Xs d×M×n (None: constant latent models), mean_Xs n×M, mean_grad n×d×M.
    Returns (mu[n, M], var[n, M], dmu[n, d, M], dvar[n, d, M]).  DomainError (with .bad_index) as GibbsGP.predict_grad."""
    gps = list(gps)
    n = len(gps)
    if n < 1:
        raise BossError(BOSS_E_INVALID, "at least one posterior is needed")
    d = gps[0].d
    Xs, lam, amp, dl, da, ms, mg = _ngp_grad_set_args(n, d, Xs, lam_Xs, amp_Xs, dlam_Xs, damp_Xs, mean_Xs, mean_grad)
    M = Xs.shape[1]
    arr = (C.c_void_p * n)(*[g._h.value for g in gps])
    mu, var = np.zeros((n, M)), np.zeros((n, M))
    dmu, dvar = np.zeros((n, M, d)), np.zeros((n, M, d))
    bad = C.c_long(-1)
    rc = load_library().boss_ngp_predict_grad_set(n, arr, M, _dp(Xs), _dp(lam), _dp(amp), _dp(dl), _dp(da), _dp(ms), _dp(mg), _dp(mu),
                                                  _dp(var), _dp(dmu), _dp(dvar), C.byref(bad))
    if rc == BOSS_E_NEG_VAR:
        e = DomainError(rc, load_library().boss_last_error().decode())
        e.bad_index = bad.value
        raise e
    _check(rc)
    return mu, var, dmu.transpose(0, 2, 1), dvar.transpose(0, 2, 1)


def ngp_acq_ei_grad_set(gps: Sequence[Sequence["GibbsGP"]], Xs, lam_Xs, amp_Xs, dlam_Xs=None, damp_Xs=None, fit_coefs=None, y_max=None,
                        best=None, valid_mask=None, mean_Xs=None, mean_grad=None):
    """EI·feas and its gradient w.r.t. the candidates for nonstationary posteriors, averaged over S hyper-parameter samples in ONE
    device call (boss_ngp_acq_ei_grad_set).  gps[s][p] = output p of sample s; the latent arrays are those of ngp_predict_grad_set
    with member i = p + P·s.  Returns (acq[M], dacq[d, M]) = the means over s of acq_ei_grad_moments on the P members'
    GibbsGP.predict_grad results."""
    S = len(gps)
    P = len(gps[0]) if S else 0
    if S < 1 or P < 1 or any(len(row) != P for row in gps):
        raise BossError(BOSS_E_INVALID, "gps must be S rows of P posteriors")
    if fit_coefs is None:
        raise BossError(BOSS_E_INVALID, "fit_coefs is needed")
    n = P * S
    d = gps[0][0].d
    Xs, lam, amp, dl, da, ms, mg = _ngp_grad_set_args(n, d, Xs, lam_Xs, amp_Xs, dlam_Xs, damp_Xs, mean_Xs, mean_grad)
    M = Xs.shape[1]
    arr = (C.c_void_p * n)()
    for s in range(S):
        for p in range(P):
            arr[p + P * s] = gps[s][p]._h
    coefs = _f64(np.asarray(fit_coefs).reshape(-1), 1)
    if coefs.shape[0] != P:
        raise BossError(BOSS_E_INVALID, "fit_coefs must have one entry per output")
    ym = None if y_max is None else _f64(np.asarray(y_max).reshape(-1), 1)
    if ym is not None and ym.shape[0] != P:
        raise BossError(BOSS_E_INVALID, "y_max must have one entry per output")
    mask = None if valid_mask is None else np.ascontiguousarray(np.asarray(valid_mask, dtype=bool).astype(np.uint8))
    if mask is not None and mask.shape != (M,):
        raise BossError(BOSS_E_INVALID, "valid_mask must have one entry per candidate")
    acq = np.zeros(M)
    dacq = np.zeros((d, M), order="F")
    _check(load_library().boss_ngp_acq_ei_grad_set(P, S, arr, M, _dp(Xs), _dp(lam), _dp(amp), _dp(dl), _dp(da), _dp(ms), _dp(mg),
                                                   _dp(coefs), _dp(ym), 0 if best is None else 1, 0.0 if best is None else float(best),
                                                   _ucp(mask), _dp(acq), _dp(dacq)))
    return acq, dacq


def acq_ei_moments(mu, var, fit_coefs, y_max=None, best=None, valid_mask=None, device: int = 0):
    """EI·feas + arg-max from posterior moments already on the host (outputs fitted on other
    ranks).  mu, var: [S][P][M] (or [P][M] for S = 1).  Returns (acq[M], argmax, max)."""
    mu = np.asarray(mu, dtype=np.float64)
    var = np.asarray(var, dtype=np.float64)
    if mu.ndim == 2:
        mu, var = mu[None], var[None]
    S, P, M = mu.shape
    assert var.shape == mu.shape
    mu, var = np.ascontiguousarray(mu), np.ascontiguousarray(var)
    coefs = _f64(np.asarray(fit_coefs).reshape(-1), 1)
    assert coefs.shape[0] == P
    ym = None if y_max is None else _f64(np.asarray(y_max).reshape(-1), 1)
    mask = None if valid_mask is None else np.ascontiguousarray(np.asarray(valid_mask, dtype=bool).astype(np.uint8))
    acq = np.zeros(M)
    am = C.c_long(-1)
    mx = C.c_double(0.0)
    _check(load_library().boss_acq_ei_moments(device, P, S, M, _dp(mu), _dp(var), _dp(coefs), _dp(ym),
                                              0 if best is None else 1, 0.0 if best is None else float(best),
                                              _ucp(mask), _dp(acq), C.byref(am), C.byref(mx)))
    return acq, am.value, mx.value


# ---------------------------------------------------------------- fitness programs: Monte-Carlo EI of a nonlinear fitness
FIT_OPS = ("ADD", "SUB", "MUL", "DIV", "NEG", "ABS", "SQUARE", "SQRT", "EXP", "LOG", "SIN", "COS", "TANH", "POW", "MIN", "MAX")
FIT_OP = {name: i for i, name in enumerate(FIT_OPS)}                 # the BOSS_FIT_* opcodes of bosship.h
FIT_UNARY = frozenset(range(FIT_OP["NEG"], FIT_OP["TANH"] + 1))
FIT_MAX_INPUTS, FIT_MAX_CONSTS, FIT_MAX_INSTR = 16, 32, 64
ACQ_OPS = FIT_OPS + ("NORMCDF", "NORMPDF")                           # acquisition programs alone know the last two (BOSS_ACQ_*)
ACQ_OP = {name: i for i, name in enumerate(ACQ_OPS)}
ACQ_MAX_OUTPUTS, ACQ_MAX_SCALARS = 8, 16


def _normcdf(z):
    from scipy.special import erfc
    return 0.5 * erfc(-z * 0.7071067811865476)


def _normpdf(z):
    return np.exp(-0.5 * z * z) * 0.3989422804014327


class FitnessProgram:
    """A fitness y -> f(y) as a straight-line program (boss_fit_t): value ids 0..P-1 are the inputs, P..P+C-1 the constants,
    P+C+i the result of instruction i = (op, a, b) on earlier ids (b = -1 on unary ops); the value is `out_id`.
    Creating one needs no device.  eval / grad are vectorised numpy interpreters of the program, eval_host runs the
    library's own interpreter (the function the kernels call) on the host."""

    def __init__(self, P: int, consts, code, out_id: int):
        self.P = int(P)
        self.consts = np.ascontiguousarray(np.asarray(consts, dtype=np.float64).reshape(-1))
        self.code = np.ascontiguousarray(np.asarray(code, dtype=np.intc).reshape(-1, 3))
        self.out_id = int(out_id)
        self._h = C.c_void_p()
        _check(load_library().boss_fit_create(self.P, self.consts.shape[0], _dp(self.consts), self.code.shape[0],
                                              self.code.ctypes.data_as(C.POINTER(C.c_int)), self.out_id, C.byref(self._h)))

    @classmethod
    def _interpreter(cls, P: int, consts, code, out_id: int) -> "FitnessProgram":
        """The numpy interpreter (eval / grad) of a program without a library handle: one output of a MeanProgram, whose d + T
        inputs may exceed what boss_fit_create takes (the MeanProgram's own handle validates it)."""
        self = cls.__new__(cls)
        self.P = int(P)
        self.consts = np.ascontiguousarray(np.asarray(consts, dtype=np.float64).reshape(-1))
        self.code = np.ascontiguousarray(np.asarray(code, dtype=np.intc).reshape(-1, 3))
        self.out_id = int(out_id)
        self._h = C.c_void_p()
        return self

    def _inputs(self, Y):
        Y = np.asarray(Y, dtype=np.float64)
        one = Y.ndim == 1
        Y = Y.reshape(self.P, -1)
        return Y, one

    def _forward(self, Y):
        n = Y.shape[1]
        vals = [Y[p] for p in range(self.P)] + [np.full(n, c) for c in self.consts]
        with np.errstate(all="ignore"):
            for op, a, b in self.code:
                x = vals[a]
                z = vals[b] if b >= 0 else None
                name = ACQ_OPS[op]                           # (NORMCDF / NORMPDF: an AcqProgram alone holds them)
                if name == "ADD": r = x + z
                elif name == "SUB": r = x - z
                elif name == "MUL": r = x * z
                elif name == "DIV": r = x / z
                elif name == "NEG": r = -x
                elif name == "ABS": r = np.abs(x)
                elif name == "SQUARE": r = x * x
                elif name == "SQRT": r = np.sqrt(x)
                elif name == "EXP": r = np.exp(x)
                elif name == "LOG": r = np.log(x)
                elif name == "SIN": r = np.sin(x)
                elif name == "COS": r = np.cos(x)
                elif name == "TANH": r = np.tanh(x)
                elif name == "POW": r = np.power(x, z)
                elif name == "MIN": r = np.where(np.isnan(x) | np.isnan(z), x + z, np.where(x <= z, x, z))
                elif name == "NORMCDF": r = _normcdf(x)
                elif name == "NORMPDF": r = _normpdf(x)
                else: r = np.where(np.isnan(x) | np.isnan(z), x + z, np.where(x >= z, x, z))
                vals.append(r)
        return vals

    def eval(self, Y):
        """f at the columns of Y (P×n, or one point of length P)."""
        Y, one = self._inputs(Y)
        f = self._forward(Y)[self.out_id]
        return float(f[0]) if one else np.array(f)

    def grad(self, Y):
        """df/dy at the columns of Y: P×n (the conventions of bosship.h: ABS'(0) = 0, MIN / MAX ties to the first operand, the
        d/db term of POW dropped for a constant exponent, an instruction with adjoint 0 passes nothing on)."""
        Y, one = self._inputs(Y)
        n, P, nc = Y.shape[1], self.P, self.consts.shape[0]
        vals = self._forward(Y)
        adj = [np.zeros(n) for _ in vals]
        adj[self.out_id] = np.ones(n)
        with np.errstate(all="ignore"):
            for i in range(self.code.shape[0] - 1, -1, -1):
                op, a, b = self.code[i]
                w = adj[P + nc + i]
                x, r = vals[a], vals[P + nc + i]
                z = vals[b] if b >= 0 else None
                name = ACQ_OPS[op]                           # (NORMCDF / NORMPDF: an AcqProgram alone holds them)
                da, db = None, None
                if name == "ADD": da, db = np.ones(n), np.ones(n)
                elif name == "SUB": da, db = np.ones(n), -np.ones(n)
                elif name == "MUL": da, db = z, x
                elif name == "DIV": da, db = 1.0 / z, -r / z
                elif name == "NEG": da = -np.ones(n)
                elif name == "ABS": da = np.sign(x)
                elif name == "SQUARE": da = 2.0 * x
                elif name == "SQRT": da = 0.5 / r
                elif name == "EXP": da = r
                elif name == "LOG": da = 1.0 / x
                elif name == "SIN": da = np.cos(x)
                elif name == "COS": da = -np.sin(x)
                elif name == "TANH": da = 1.0 - r * r
                elif name == "POW":
                    da = z * np.power(x, z - 1.0)
                    db = np.zeros(n) if P <= b < P + nc else r * np.log(x)
                elif name == "MIN": da, db = (x <= z).astype(float), (~(x <= z)).astype(float)
                elif name == "NORMCDF": da = _normpdf(x)
                elif name == "NORMPDF": da = -x * r
                else: da, db = (x >= z).astype(float), (~(x >= z)).astype(float)
                adj[a] = adj[a] + np.where(w == 0.0, 0.0, w * da)
                if db is not None:
                    adj[b] = adj[b] + np.where(w == 0.0, 0.0, w * db)
        g = np.stack(adj[:P])
        return g[:, 0] if one else g

    def eval_host(self, Y, want_grad: bool = False):
        """The same through boss_fit_eval_host.  Returns f[n], or (f[n], df[P, n]) with want_grad."""
        Y, one = self._inputs(Y)
        Yf = np.asfortranarray(Y)
        n = Yf.shape[1]
        f = np.zeros(n)
        df = np.zeros((self.P, n), order="F") if want_grad else None
        _check(load_library().boss_fit_eval_host(self._h, n, _dp(Yf), _dp(f), _dp(df)))
        if one:
            return (float(f[0]), df[:, 0]) if want_grad else float(f[0])
        return (f, df) if want_grad else f

    def close(self):
        if self._h:
            load_library().boss_fit_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------- kernel programs: a user-defined covariance function
KERN_MAX_DIM = 16                                                    # two points of up to 16 dimensions: 32 inputs


class KernelProgram:
    """A covariance function (u, v) -> k as a straight-line program (boss_kern_t): the layout of a FitnessProgram over 2·d inputs,
    u[0..d) first, then v[0..d).  Creating one needs no device.  eval is the vectorised numpy interpreter, eval_host runs the
    library's own interpreter (the function the kernels call) on the host."""

    def __init__(self, d: int, consts, code, out_id: int):
        self.d = int(d)
        self.consts = np.ascontiguousarray(np.asarray(consts, dtype=np.float64).reshape(-1))
        self.code = np.ascontiguousarray(np.asarray(code, dtype=np.intc).reshape(-1, 3))
        self.out_id = int(out_id)
        self._h = C.c_void_p()
        _check(load_library().boss_kern_create(self.d, self.consts.shape[0], _dp(self.consts), self.code.shape[0],
                                               self.code.ctypes.data_as(C.POINTER(C.c_int)), self.out_id, C.byref(self._h)))
        self._interp = FitnessProgram._interpreter(2 * self.d, self.consts, self.code, self.out_id)

    def _pairs(self, U, V):
        U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
        one = U.ndim == 1
        U, V = U.reshape(self.d, -1), V.reshape(self.d, -1)
        if U.shape != V.shape:
            raise ValueError("U and V must hold the same number of points")
        return U, V, one

    def eval(self, U, V):
        """k(U[:, j], V[:, j]) for every column j (d×n each, or two points of length d)."""
        U, V, one = self._pairs(U, V)
        k = self._interp.eval(np.vstack([U, V]))
        return float(k[0]) if one else k

    def eval_host(self, U, V):
        """The same through boss_kern_eval_host."""
        U, V, one = self._pairs(U, V)
        Uf, Vf = np.asfortranarray(U), np.asfortranarray(V)
        k = np.zeros(Uf.shape[1])
        _check(load_library().boss_kern_eval_host(self._h, Uf.shape[1], _dp(Uf), _dp(Vf), _dp(k)))
        return float(k[0]) if one else k

    def grad(self, U, V):
        """(k, dU, dV) through boss_kern_grad_host: the program's value and its partials ∂f/∂u, ∂f/∂v (d×n each, or length d for two
        points) by the reverse sweep the gradient kernels run; a local partial of exactly 0 passes 0 on (finite at coincident
        points)."""
        U, V, one = self._pairs(U, V)
        Uf, Vf = np.asfortranarray(U), np.asfortranarray(V)
        n = Uf.shape[1]
        k, dU, dV = np.zeros(n), np.zeros((self.d, n), order="F"), np.zeros((self.d, n), order="F")
        _check(load_library().boss_kern_grad_host(self._h, n, _dp(Uf), _dp(Vf), _dp(k), _dp(dU), _dp(dV)))
        return (float(k[0]), dU[:, 0].copy(), dV[:, 0].copy()) if one else (k, dU, dV)

    def close(self):
        if self._h:
            load_library().boss_kern_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KernelGP(GP):
    """One output slice's posterior under a KernelProgram (boss_kgp_create): update, sync, predict, set_y, factor and acq_ei work as
    for a GP; every other call of the base class is refused by the library (BOSS_E_INVALID, "program-kernel posteriors").
    grad=True (boss_kgp_set_grad) adds loglike_grad, loglike_grad_mean, predict_grad, acq_ei_grad and acq_ei_grad_set.
    sequential=True (boss_kgp_set_sequential) adds append, reserve and Track(gp, cand) with acq_ei_tracks."""

    def __init__(self, X, y, kern: KernelProgram, discrete=None, device: int = 0, grad: bool = False, sequential: bool = False):
        lib = load_library()
        X = _f64(X, 2)
        y = _f64(np.asarray(y).reshape(-1), 1)
        self.d, self.N = X.shape
        if y.shape[0] != self.N:
            raise ValueError("y must have one entry per column of X")
        if not isinstance(kern, KernelProgram):
            raise TypeError("kern must be a KernelProgram")
        self.device = device
        self.kernel = kern
        disc = None if discrete is None else np.ascontiguousarray(np.asarray(discrete, dtype=bool).astype(np.uint8))
        h = C.c_void_p()
        _check(lib.boss_kgp_create(device, self.d, self.N, _dp(X), _dp(y), _ucp(disc), kern._h, C.byref(h)))
        self._h = h
        self.logpdf = None
        self.grad = bool(grad)
        self.sequential = bool(sequential)
        try:
            if self.grad:
                _check(lib.boss_kgp_set_grad(self._h, 1))
            if self.sequential:
                _check(lib.boss_kgp_set_sequential(self._h, 1))
        except Exception:
            self.close()
            raise


def _kgp_batch_args(X, y, kern, lengthscales, amplitudes, noise_stds, mean_X, discrete):
    """The arrays boss_kgp_loglike_batch / boss_kgp_fit_batch read, converted and checked (no device is touched): X d×N, y N,
    lengthscales d×S, amplitudes / noise_stds S, mean_X None, N values or S×N rows."""
    if not isinstance(kern, KernelProgram):
        raise TypeError("kern must be a KernelProgram")
    X = _f64(X, 2)
    y = _f64(np.asarray(y).reshape(-1), 1)
    lam = _f64(lengthscales, 2)
    d, N = X.shape
    S = lam.shape[1]
    if lam.shape[0] != d:
        raise BossError(BOSS_E_INVALID, "lengthscales must be d×S")
    amp = _f64(np.asarray(amplitudes).reshape(-1), 1)
    sig = _f64(np.asarray(noise_stds).reshape(-1), 1)
    if amp.shape[0] != S or sig.shape[0] != S:
        raise BossError(BOSS_E_INVALID, "amplitudes and noise_stds must have one entry per set")
    if y.shape[0] != N:
        raise ValueError("y must have one entry per column of X")
    stride, m = 0, None
    if mean_X is not None:
        m = np.asarray(mean_X, dtype=np.float64)
        if m.ndim == 2:
            if m.shape != (S, N):
                raise ValueError("mean_X must be S×N (one prior-mean row per set) or a vector of N entries")
            m, stride = np.ascontiguousarray(m), N
        else:
            m = np.ascontiguousarray(m.reshape(-1))
            if m.shape[0] != N:
                raise ValueError("mean_X must be S×N (one prior-mean row per set) or a vector of N entries")
    disc = None if discrete is None else np.ascontiguousarray(np.asarray(discrete, dtype=bool).astype(np.uint8))
    return X, y, lam, amp, sig, m, stride, disc, d, N, S


def kgp_loglike_batch(X, y, kern: KernelProgram, lengthscales, amplitudes, noise_stds, mean_X=None, discrete=None, device: int = 0):
    """S log marginal likelihoods of one output slice under a KernelProgram in one call (boss_kgp_loglike_batch); lengthscales is
    d×S.  Returns (ll[S], status[S]); ll = -Inf where a set is invalid or its matrix is not PD (safe_data_loglike).  Every value is
    bit for bit the logpdf of KernelGP.update at the same parameters."""
    X, y, lam, amp, sig, m, stride, disc, d, N, S = _kgp_batch_args(X, y, kern, lengthscales, amplitudes, noise_stds, mean_X, discrete)
    ll = np.zeros(S)
    st = np.zeros(S, dtype=np.int32)
    _check(load_library().boss_kgp_loglike_batch(device, d, N, _dp(X), _dp(y), _ucp(disc), kern._h, S, _dp(lam), _dp(amp), _dp(sig),
                                                 _dp(m), stride, _dp(ll), st.ctypes.data_as(C.POINTER(C.c_int))))
    return ll, st


def kgp_fit_batch(X, y, kern: KernelProgram, lengthscales, amplitudes, noise_stds, mean_X=None, discrete=None, device: int = 0,
                  grad: bool = False, sequential: bool = False):
    """S resident posteriors of one output slice under a KernelProgram from ONE batched factorisation (boss_kgp_fit_batch): what
    model_posterior builds per sample of a BI fit (src/posterior.jl:15-19).  Returns (gps[S], logpdf[S], status[S]): KernelGP
    members of one set (grad=True: boss_kgp_set_grad on each, sequential=True: boss_kgp_set_sequential on each); members with
    status != 0 are unfitted handles."""
    X, y, lam, amp, sig, m, stride, disc, d, N, S = _kgp_batch_args(X, y, kern, lengthscales, amplitudes, noise_stds, mean_X, discrete)
    if not (np.isfinite(amp).all() and np.isfinite(sig).all() and np.isfinite(lam).all()):
        raise BossError(BOSS_E_INVALID, "hyper-parameters must be finite")
    lib = load_library()
    hs = (C.c_void_p * max(S, 1))()
    ll = np.zeros(S)
    st = np.zeros(S, dtype=np.int32)
    _check(lib.boss_kgp_fit_batch(device, kern._h, d, N, _dp(X), _dp(y), _dp(m), stride, _ucp(disc), S, _dp(lam), _dp(amp), _dp(sig),
                                  hs, _dp(ll), st.ctypes.data_as(C.POINTER(C.c_int))))
    gps = []
    for s in range(S):
        g = KernelGP.__new__(KernelGP)
        g.d, g.N, g.device, g.kernel, g._h = d, N, device, kern, C.c_void_p(hs[s])
        g.logpdf = float(ll[s]) if st[s] == 0 else None
        g.grad = g.sequential = False
        gps.append(g)
    if grad or sequential:
        try:
            for g in gps:
                if grad:
                    _check(lib.boss_kgp_set_grad(g._h, 1))
                    g.grad = True
                if sequential:
                    _check(lib.boss_kgp_set_sequential(g._h, 1))
                    g.sequential = True
        except Exception:
            for g in gps:
                g.close()
            raise
    return gps, ll, st


def _mc_common(fit: FitnessProgram, eps, y_max, valid_mask):
    eps = _f64(eps, 2)                                           # P×n_eps, one ε-sample per column
    ym = None if y_max is None else _f64(np.asarray(y_max).reshape(-1), 1)
    mask = None if valid_mask is None else np.ascontiguousarray(np.asarray(valid_mask, dtype=bool).astype(np.uint8))
    return eps, ym, mask


def acq_ei_mc(gps: Sequence[Sequence[GP]], cand: Candidates, fit: FitnessProgram, eps, y_max=None, best=None, valid_mask=None,
              mean_Xs=None, want_acq: bool = True):
    """acq_ei with the Monte-Carlo EI of a fitness program (boss_acq_ei_mc): eps P×K for one posterior sample, P×S for S > 1
    (sample s takes column s).  Returns (acq[M] or None, argmax, max)."""
    S = len(gps)
    P = len(gps[0])
    arr = (C.c_void_p * (P * S))()
    for s in range(S):
        for p in range(P):
            arr[p + P * s] = gps[s][p]._h
    eps, ym, mask = _mc_common(fit, eps, y_max, valid_mask)
    M = cand.M
    ms = None
    if mean_Xs is not None:
        a = np.asarray(mean_Xs, dtype=np.float64).reshape(S, P, M)
        ms = np.ascontiguousarray(a.transpose(0, 2, 1))       # index p + P*(j + M*s)
    acq = np.zeros(M) if want_acq else None
    am = C.c_long(-1)
    mx = C.c_double(0.0)
    _check(load_library().boss_acq_ei_mc(P, S, arr, cand._h, _dp(ms), fit._h, eps.shape[1], _dp(eps), _dp(ym), 0 if best is None else 1,
                                         0.0 if best is None else float(best), _ucp(mask), _dp(acq), C.byref(am), C.byref(mx)))
    return acq, am.value, mx.value


def acq_ei_mc_moments(mu, var, fit: FitnessProgram, eps, y_max=None, best=None, valid_mask=None, device: int = 0):
    """acq_ei_moments with the Monte-Carlo EI of a fitness program (boss_acq_ei_mc_moments).  mu, var: [S][P][M] (or [P][M])."""
    mu = np.asarray(mu, dtype=np.float64)
    var = np.asarray(var, dtype=np.float64)
    if mu.ndim == 2:
        mu, var = mu[None], var[None]
    S, P, M = mu.shape
    if var.shape != mu.shape:
        raise ValueError("mu and var must have one shape")
    mu, var = np.ascontiguousarray(mu), np.ascontiguousarray(var)
    eps, ym, mask = _mc_common(fit, eps, y_max, valid_mask)
    acq = np.zeros(M)
    am = C.c_long(-1)
    mx = C.c_double(0.0)
    _check(load_library().boss_acq_ei_mc_moments(device, P, S, M, _dp(mu), _dp(var), fit._h, eps.shape[1], _dp(eps), _dp(ym),
                                                 0 if best is None else 1, 0.0 if best is None else float(best), _ucp(mask), _dp(acq),
                                                 C.byref(am), C.byref(mx)))
    return acq, am.value, mx.value


def acq_ei_mc_grad(gps: Sequence[Sequence[GP]], Xs, fit: FitnessProgram, eps, y_max=None, best=None, valid_mask=None, mean_Xs=None,
                   mean_grad=None):
    """acq_ei_grad_set with the Monte-Carlo EI of a fitness program (boss_acq_ei_mc_grad); S = 1 included.  gps[s][p];
    mean_Xs None or [S][P][M]; mean_grad None or [S][P][d][M].  Returns (acq[M], dacq[d, M])."""
    S = len(gps)
    P = len(gps[0]) if S else 0
    if S < 1 or P < 1 or any(len(row) != P for row in gps):
        raise BossError(BOSS_E_INVALID, "gps must be S rows of P posteriors")
    Xs = _f64(Xs, 2)
    d, M = Xs.shape
    arr = (C.c_void_p * (P * S))()
    for s in range(S):
        for p in range(P):
            arr[p + P * s] = gps[s][p]._h
    eps, ym, mask = _mc_common(fit, eps, y_max, valid_mask)
    ms = None if mean_Xs is None else np.ascontiguousarray(np.asarray(mean_Xs, dtype=np.float64).reshape(S, P, M))
    mg = None
    if mean_grad is not None:
        a = np.asarray(mean_grad, dtype=np.float64).reshape(S, P, d, M)
        mg = np.ascontiguousarray(a.transpose(0, 1, 3, 2))        # [s][p][j*d + m]
    acq = np.zeros(M)
    dacq = np.zeros((d, M), order="F")
    _check(load_library().boss_acq_ei_mc_grad(P, S, arr, M, _dp(Xs), _dp(ms), _dp(mg), fit._h, eps.shape[1], _dp(eps), _dp(ym),
                                              0 if best is None else 1, 0.0 if best is None else float(best), _ucp(mask), _dp(acq),
                                              _dp(dacq)))
    return acq, dacq


def acq_ei_mc_grad_moments(mu, var, dmu, dvar, fit: FitnessProgram, eps, y_max=None, best=None, valid_mask=None, device: int = 0):
    """acq_ei_grad_moments over S posterior samples with the Monte-Carlo EI of a fitness program (boss_acq_ei_mc_grad_moments):
    mu / var [S][P][M] (or [P][M]), dmu / dvar [S][P][d][M].  Returns (acq[M], dacq[d, M])."""
    mu = np.asarray(mu, dtype=np.float64)
    var = np.asarray(var, dtype=np.float64)
    if mu.ndim == 2:
        mu, var = mu[None], var[None]
    S, P, M = mu.shape
    if var.shape != mu.shape:
        raise ValueError("mu and var must have one shape")
    mu, var = np.ascontiguousarray(mu), np.ascontiguousarray(var)
    gm = np.asarray(dmu, dtype=np.float64).reshape(S, P, -1, M)
    gv = np.asarray(dvar, dtype=np.float64).reshape(S, P, -1, M)
    d = gm.shape[2]
    gm = np.ascontiguousarray(gm.transpose(0, 1, 3, 2))           # [s][p][j*d + m]
    gv = np.ascontiguousarray(gv.transpose(0, 1, 3, 2))
    eps, ym, mask = _mc_common(fit, eps, y_max, valid_mask)
    acq = np.zeros(M)
    dacq = np.zeros((d, M), order="F")
    _check(load_library().boss_acq_ei_mc_grad_moments(device, P, S, M, d, _dp(mu), _dp(var), _dp(gm), _dp(gv), fit._h, eps.shape[1],
                                                      _dp(eps), _dp(ym), 0 if best is None else 1, 0.0 if best is None else float(best),
                                                      _ucp(mask), _dp(acq), _dp(dacq)))
    return acq, dacq


# ---------------------------------------------------------------- acquisition programs: a user-defined acquisition on the device
class AcqProgram(FitnessProgram):
    """An acquisition (mu, var, q) -> value as a straight-line program (boss_acqp_t) over 2P + Q inputs: value ids 0..P-1 are the
    posterior means, P..2P-1 the (clipped) variances, 2P..2P+Q-1 the runtime scalars; then constants and instructions as in a
    FitnessProgram, with the two extra unary opcodes NORMCDF / NORMPDF (ACQ_OPS).  Creating one needs no device.  eval / grad
    (inherited) are the numpy interpreters over the stacked inputs [mu; var; q]; eval_host runs the library's interpreter."""

    def __init__(self, y_dim: int, n_params: int, consts, code, out_id: int):
        self.y_dim, self.n_params = int(y_dim), int(n_params)
        self.P = 2 * self.y_dim + self.n_params               # (the interpreter's input count)
        self.consts = np.ascontiguousarray(np.asarray(consts, dtype=np.float64).reshape(-1))
        self.code = np.ascontiguousarray(np.asarray(code, dtype=np.intc).reshape(-1, 3))
        self.out_id = int(out_id)
        self._h = C.c_void_p()
        _check(load_library().boss_acqp_create(self.y_dim, self.n_params, self.consts.shape[0], _dp(self.consts), self.code.shape[0],
                                               self.code.ctypes.data_as(C.POINTER(C.c_int)), self.out_id, C.byref(self._h)))

    def scalars(self, q):
        q = np.zeros(0) if q is None else np.ascontiguousarray(np.asarray(q, dtype=np.float64).reshape(-1))
        if q.shape[0] != self.n_params:
            raise ValueError(f"the acquisition program takes {self.n_params} runtime scalars, got {q.shape[0]}")
        return q

    def stack(self, mu, var, q=None):
        """[mu; var; q] as the P×n input block of eval / grad (mu, var: y_dim×n or length y_dim)."""
        mu = np.asarray(mu, dtype=np.float64).reshape(self.y_dim, -1)
        var = np.asarray(var, dtype=np.float64).reshape(self.y_dim, -1)
        q = self.scalars(q)
        return np.vstack([mu, var, np.repeat(q[:, None], mu.shape[1], axis=1)])

    def eval_host(self, mu, var, q=None, want_grad: bool = False):
        """The raw program (no clip, no mask) through boss_acqp_eval_host at the columns of mu / var (y_dim×n).  Returns a[n], or
        (a[n], da_dmu[y_dim, n], da_dvar[y_dim, n]) with want_grad."""
        mu = np.asfortranarray(np.asarray(mu, dtype=np.float64).reshape(self.y_dim, -1))
        var = np.asfortranarray(np.asarray(var, dtype=np.float64).reshape(self.y_dim, -1))
        q = self.scalars(q)
        n = mu.shape[1]
        a = np.zeros(n)
        dm = np.zeros((self.y_dim, n), order="F") if want_grad else None
        dv = np.zeros((self.y_dim, n), order="F") if want_grad else None
        _check(load_library().boss_acqp_eval_host(self._h, n, _dp(mu), _dp(var), _dp(q) if q.shape[0] else None, _dp(a), _dp(dm), _dp(dv)))
        return (a, dm, dv) if want_grad else a

    def close(self):
        if self._h:
            load_library().boss_acqp_free(self._h)
            self._h = C.c_void_p()


def _handles(gps):
    S = len(gps)
    P = len(gps[0]) if S else 0
    if S < 1 or P < 1 or any(len(row) != P for row in gps):
        raise BossError(BOSS_E_INVALID, "gps must be S rows of P posteriors")
    arr = (C.c_void_p * (P * S))()
    for s in range(S):
        for p in range(P):
            arr[p + P * s] = gps[s][p]._h
    return S, P, arr


def _mask_u8(valid_mask):
    return None if valid_mask is None else np.ascontiguousarray(np.asarray(valid_mask, dtype=bool).astype(np.uint8))


def acq_prog(gps: Sequence[Sequence[GP]], cand: Candidates, prog: AcqProgram, q=None, valid_mask=None, outside: float = -np.inf,
             mean_Xs=None, want_acq: bool = True):
    """The acquisition program behind the prediction of gps[s][p] at resident candidates (boss_acq_prog): sample mean, mask to
    `outside`, first-index arg-max.  mean_Xs None or [S][P][M].  Returns (acq[M] or None, argmax, max)."""
    S, P, arr = _handles(gps)
    q = prog.scalars(q)
    M = cand.M
    ms = None
    if mean_Xs is not None:
        ms = np.ascontiguousarray(np.asarray(mean_Xs, dtype=np.float64).reshape(S, P, M).transpose(0, 2, 1))   # index p + P*(j + M*s)
    mask = _mask_u8(valid_mask)
    acq = np.zeros(M) if want_acq else None
    am = C.c_long(-1)
    mx = C.c_double(0.0)
    _check(load_library().boss_acq_prog(P, S, arr, cand._h, _dp(ms), prog._h, _dp(q) if q.shape[0] else None, _ucp(mask), float(outside),
                                        _dp(acq), C.byref(am), C.byref(mx)))
    return acq, am.value, mx.value


def _moments(mu, var):
    mu = np.asarray(mu, dtype=np.float64)
    var = np.asarray(var, dtype=np.float64)
    if mu.ndim == 2:
        mu, var = mu[None], var[None]
    if var.shape != mu.shape:
        raise ValueError("mu and var must have one shape")
    return np.ascontiguousarray(mu), np.ascontiguousarray(var)


def acq_prog_moments(mu, var, prog: AcqProgram, q=None, valid_mask=None, outside: float = -np.inf, device: int = 0):
    """acq_prog from moments on the host (boss_acq_prog_moments).  mu, var: [S][P][M] (or [P][M])."""
    mu, var = _moments(mu, var)
    S, P, M = mu.shape
    q = prog.scalars(q)
    mask = _mask_u8(valid_mask)
    acq = np.zeros(M)
    am = C.c_long(-1)
    mx = C.c_double(0.0)
    _check(load_library().boss_acq_prog_moments(device, P, S, M, _dp(mu), _dp(var), prog._h, _dp(q) if q.shape[0] else None, _ucp(mask),
                                                float(outside), _dp(acq), C.byref(am), C.byref(mx)))
    return acq, am.value, mx.value


def acq_prog_grad(gps: Sequence[Sequence[GP]], Xs, prog: AcqProgram, q=None, valid_mask=None, outside: float = -np.inf, mean_Xs=None,
                  mean_grad=None):
    """Value and gradient w.r.t. the candidates of the acquisition program, averaged over the S samples (boss_acq_prog_grad).
    gps[s][p]; mean_Xs None or [S][P][M]; mean_grad None or [S][P][d][M].  Returns (acq[M], dacq[d, M])."""
    S, P, arr = _handles(gps)
    Xs = _f64(Xs, 2)
    d, M = Xs.shape
    q = prog.scalars(q)
    mask = _mask_u8(valid_mask)
    ms = None if mean_Xs is None else np.ascontiguousarray(np.asarray(mean_Xs, dtype=np.float64).reshape(S, P, M))
    mg = None
    if mean_grad is not None:
        mg = np.ascontiguousarray(np.asarray(mean_grad, dtype=np.float64).reshape(S, P, d, M).transpose(0, 1, 3, 2))   # [s][p][j*d + m]
    acq = np.zeros(M)
    dacq = np.zeros((d, M), order="F")
    _check(load_library().boss_acq_prog_grad(P, S, arr, M, _dp(Xs), _dp(ms), _dp(mg), prog._h, _dp(q) if q.shape[0] else None, _ucp(mask),
                                             float(outside), _dp(acq), _dp(dacq)))
    return acq, dacq


def acq_prog_grad_moments(mu, var, dmu, dvar, prog: AcqProgram, q=None, valid_mask=None, outside: float = -np.inf, device: int = 0):
    """acq_prog_grad from moments and moment gradients on the host (boss_acq_prog_grad_moments): mu / var [S][P][M] (or [P][M]),
    dmu / dvar [S][P][d][M].  Returns (acq[M], dacq[d, M])."""
    mu, var = _moments(mu, var)
    S, P, M = mu.shape
    gm = np.asarray(dmu, dtype=np.float64).reshape(S, P, -1, M)
    gv = np.asarray(dvar, dtype=np.float64).reshape(S, P, -1, M)
    d = gm.shape[2]
    gm = np.ascontiguousarray(gm.transpose(0, 1, 3, 2))           # [s][p][j*d + m]
    gv = np.ascontiguousarray(gv.transpose(0, 1, 3, 2))
    q = prog.scalars(q)
    mask = _mask_u8(valid_mask)
    acq = np.zeros(M)
    dacq = np.zeros((d, M), order="F")
    _check(load_library().boss_acq_prog_grad_moments(device, P, S, M, d, _dp(mu), _dp(var), _dp(gm), _dp(gv), prog._h,
                                                     _dp(q) if q.shape[0] else None, _ucp(mask), float(outside), _dp(acq), _dp(dacq)))
    return acq, dacq


# ---------------------------------------------------------------- mean programs: the parametric mean and its Jacobians on the device
MEAN_MAX_INPUTS, MEAN_MAX_CONSTS, MEAN_MAX_INSTR, MEAN_MAX_OUTPUTS = 32, 32, 64, 16
MEAN_SAMPLE_MAJOR, MEAN_OUTPUT_MAJOR = 0, 1                          # the `layout` of boss_mean_eval


class MeanProgram:
    """The mean (x, θ) -> length-P vector as P straight-line programs over the shared inputs x (d) and θ (T) (boss_mean_t).
    outputs: per output (consts, code, out_id) as FitnessProgram takes them, with value ids 0..d-1 = x, d..d+T-1 = θ.
    Creating one needs no device.  eval / jac are numpy interpreters (FitnessProgram.eval / grad per output), eval_host runs the
    library's interpreter on the host, eval_device the kernel (boss_mean_eval): all points, outputs and θ sets in one call.

    Shapes returned by eval_host / eval_device, with B = (S, P) for layout 0 (sample-major) and (P, S) for layout 1:
    m B×n, jac_theta B×n×T, jac_x B×d×n — views of the blocks the C ABI fills (jac_theta[b] is n×T column-major, jac_x[b] d×n
    column-major)."""

    def __init__(self, d: int, T: int, outputs):
        self.d, self.T, self.P = int(d), int(T), len(outputs)
        self.outputs = [FitnessProgram._interpreter(self.d + self.T, c, k, o) for c, k, o in outputs]
        nc = np.array([q.consts.shape[0] for q in self.outputs], dtype=np.intc)
        ni = np.array([q.code.shape[0] for q in self.outputs], dtype=np.intc)
        consts = np.ascontiguousarray(np.concatenate([q.consts for q in self.outputs] + [np.zeros(0)]))
        code = np.ascontiguousarray(np.concatenate([q.code.reshape(-1) for q in self.outputs] + [np.zeros(0, dtype=np.intc)]).astype(np.intc))
        outs = np.array([q.out_id for q in self.outputs], dtype=np.intc)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        self._h = C.c_void_p()
        _check(load_library().boss_mean_create(self.d, self.T, self.P, ip(nc), _dp(consts), ip(ni), ip(code), ip(outs), C.byref(self._h)))

    def _args(self, X, thetas):
        X = np.asfortranarray(X, dtype=np.float64)
        if X.ndim == 1:
            X = np.asfortranarray(X[:, None])
        if X.ndim != 2 or X.shape[0] != self.d:
            raise ValueError(f"X must be {self.d}×n")
        if self.T == 0:
            if thetas is not None and np.size(thetas):
                raise ValueError("this mean program takes no parameters (T = 0)")
            return X, None, 1
        th = np.asarray(thetas, dtype=np.float64)
        if th.ndim == 1:
            th = th[:, None]
        if th.ndim != 2 or th.shape[0] != self.T:
            raise ValueError(f"thetas must be {self.T}×S (one parameter set per column)")
        return X, np.asfortranarray(th), th.shape[1]

    def _Y(self, X, th, s):
        n = X.shape[1]
        return X if th is None else np.vstack([X, np.repeat(th[:, s:s + 1], n, axis=1)])

    def eval(self, X, thetas=None):
        """m[S, P, n] by the numpy interpreter."""
        X, th, S = self._args(X, thetas)
        return np.stack([np.stack([np.asarray(q.eval(self._Y(X, th, s)), float).reshape(-1) for q in self.outputs]) for s in range(S)])

    def jac(self, X, thetas=None):
        """(∂m/∂θ [S, P, n, T], ∂m/∂x [S, P, d, n]) by the numpy reverse sweep."""
        X, th, S = self._args(X, thetas)
        G = np.stack([np.stack([q.grad(self._Y(X, th, s)).reshape(self.d + self.T, -1) for q in self.outputs]) for s in range(S)])
        return np.ascontiguousarray(G[:, :, self.d:, :].transpose(0, 1, 3, 2)), np.ascontiguousarray(G[:, :, :self.d, :])

    def _run(self, fn, head, X, thetas, layout, jac_theta, jac_x):
        X, th, S = self._args(X, thetas)
        if layout not in (MEAN_SAMPLE_MAJOR, MEAN_OUTPUT_MAJOR):
            raise BossError(BOSS_E_INVALID, "layout must be 0 (sample-major) or 1 (output-major)")
        if jac_theta and self.T == 0:
            raise BossError(BOSS_E_INVALID, "jac_theta asked of a mean program without parameters (T = 0)")
        n, P, d, T = X.shape[1], self.P, self.d, self.T
        B = (S, P) if layout == MEAN_SAMPLE_MAJOR else (P, S)
        m = np.zeros(B + (n,))
        jt = np.zeros(B + (T, n)) if jac_theta else None
        jx = np.zeros(B + (n, d)) if jac_x else None
        _check(fn(*head, self._h, n, _dp(X), S, _dp(th), layout, _dp(m), _dp(jt), _dp(jx)))
        return m, (None if jt is None else jt.transpose(0, 1, 3, 2)), (None if jx is None else jx.transpose(0, 1, 3, 2))

    def eval_host(self, X, thetas=None, layout: int = 0, jac_theta: bool = False, jac_x: bool = False):
        """(m, jac_theta or None, jac_x or None) through boss_mean_eval_host."""
        return self._run(load_library().boss_mean_eval_host, (), X, thetas, layout, jac_theta, jac_x)

    def eval_device(self, X, thetas=None, layout: int = 0, jac_theta: bool = False, jac_x: bool = False, device: int = 0):
        """(m, jac_theta or None, jac_x or None) in one device call (boss_mean_eval)."""
        return self._run(load_library().boss_mean_eval, (device,), X, thetas, layout, jac_theta, jac_x)

    def workgroup(self, n: int, grad: bool):
        """(waves per workgroup, dynamic LDS bytes) boss_mean_eval launches for n points (introspection for the tests)."""
        lib = load_library()
        lib.boss_debug_mean_block.restype = C.c_int
        lib.boss_debug_mean_block.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
        lds = C.c_int(0)
        return lib.boss_debug_mean_block(self._h, 1 if grad else 0, int(n), C.byref(lds)), lds.value

    def close(self):
        if self._h:
            load_library().boss_mean_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------- warps: input warp and output transform as device programs
WARP_MAX_DIM, WARP_MAX_OUTPUTS = 16, 8


class WarpProgram:
    """The input warp x -> x_ and the output transform (mu_, sd_) -> (mu, sd) of a transformed model (boss_warp_t).
    in_prog: None or a MeanProgram with T = 0, d = d_user inputs and d_model outputs; out_prog: None or a MeanProgram with T = 0 over
    the 2P inputs (mu_0.., sd_0..) with 2P outputs; P the number of model outputs.  The warp keeps copies: the MeanPrograms may be
    closed afterwards.  Creating one needs no device.

    apply / apply_host: Xs d_user×M -> (X_ d_model×M, J [M, d_model, d_user] or None).
    moments / moments_host: mu_, var_ [S, P, M] (or [P, M]), gradients dmu_, dvar_ [S, P, d_model, M], jac = J of apply ->
    (mu, var[, dmu, dvar [S, P, d_user, M]]).  check=True raises DomainError (.bad_index) at a variance below -1e-8; check=False
    passes such a candidate's moments through with zero gradients (the acquisition convention)."""

    def __init__(self, in_prog: Optional["MeanProgram"], P: int, out_prog: Optional["MeanProgram"]):
        self.P = int(P)
        self.d_user = None if in_prog is None else in_prog.d
        self.d_model = None if in_prog is None else in_prog.P
        self.has_out = out_prog is not None
        self._h = C.c_void_p()
        _check(load_library().boss_warp_create(None if in_prog is None else in_prog._h, self.P, None if out_prog is None else out_prog._h,
                                               C.byref(self._h)))

    def _apply(self, fn, head, Xs, jac):
        Xs = _f64(Xs, 2)
        if self.d_user is not None and Xs.shape[0] != self.d_user:
            raise ValueError(f"Xs must be {self.d_user}×M")
        M = Xs.shape[1]
        dm = self.d_model or 0
        Xo = np.zeros((dm, M), order="F")
        J = np.zeros((M, self.d_user or 0, dm)) if jac else None     # per candidate d_model×d_user column-major
        _check(fn(*head, self._h, M, _dp(Xs), _dp(Xo), _dp(J)))
        return Xo, (None if J is None else J.transpose(0, 2, 1))

    def apply_host(self, Xs, jac: bool = False):
        return self._apply(load_library().boss_warp_apply_host, (), Xs, jac)

    def apply(self, Xs, jac: bool = False, device: int = 0):
        return self._apply(load_library().boss_warp_apply, (device,), Xs, jac)

    def _moments(self, fn, head, mu_, var_, dmu_, dvar_, jac, d_user, check):
        mu_ = np.asarray(mu_, dtype=np.float64)
        var_ = np.asarray(var_, dtype=np.float64)
        squeeze = mu_.ndim == 2
        if squeeze:
            mu_, var_ = mu_[None], var_[None]
        if mu_.ndim != 3 or var_.shape != mu_.shape or mu_.shape[1] != self.P:
            raise ValueError(f"mu_ and var_ must be [S, {self.P}, M] (or [{self.P}, M])")
        S, P, M = mu_.shape
        mu_, var_ = np.ascontiguousarray(mu_), np.ascontiguousarray(var_)
        grad = dmu_ is not None
        if grad != (dvar_ is not None):
            raise ValueError("dmu_ and dvar_ come together")
        gm = gv = Jc = dmu = dvar = None
        du = self.d_user if d_user is None else int(d_user)
        if grad:
            gm = np.asarray(dmu_, dtype=np.float64).reshape(S, P, -1, M)
            gv = np.asarray(dvar_, dtype=np.float64).reshape(S, P, -1, M)
            if du is None:
                du = gm.shape[2]
            gm = np.ascontiguousarray(gm.transpose(0, 1, 3, 2))       # [s][p][j*d_model + k']
            gv = np.ascontiguousarray(gv.transpose(0, 1, 3, 2))
            if jac is not None:
                Jc = np.ascontiguousarray(np.asarray(jac, dtype=np.float64).transpose(0, 2, 1))   # [j][k][k']: d_model×d_user column-major
            dmu, dvar = np.zeros((S, P, M, du)), np.zeros((S, P, M, du))
        if du is None:
            du = 1                                                   # (no gradients, no input program: the value is not used)
        mu, var = np.zeros((S, P, M)), np.zeros((S, P, M))
        bad = C.c_long(-1)
        try:
            _check(fn(*head, self._h, S, M, du, _dp(mu_), _dp(var_), _dp(gm), _dp(gv), _dp(Jc), _dp(mu), _dp(var), _dp(dmu), _dp(dvar),
                      C.byref(bad) if check else None))
        except DomainError as e:
            e.bad_index = bad.value
            raise
        out = (mu, var) if not grad else (mu, var, dmu.transpose(0, 1, 3, 2), dvar.transpose(0, 1, 3, 2))
        return tuple(a[0] for a in out) if squeeze else out

    def moments_host(self, mu_, var_, dmu_=None, dvar_=None, jac=None, d_user=None, check: bool = True):
        return self._moments(load_library().boss_warp_moments_host, (), mu_, var_, dmu_, dvar_, jac, d_user, check)

    def moments(self, mu_, var_, dmu_=None, dvar_=None, jac=None, d_user=None, check: bool = True, device: int = 0):
        return self._moments(load_library().boss_warp_moments, (device,), mu_, var_, dmu_, dvar_, jac, d_user, check)

    # -- one-call paths: gps[s][p] fitted on model-space data, Xs d_user×M in user space; mean_Xs None or [S][P][M] (the base model's
    #    prior mean at the warped points), mean_grad None or [S][P][d_model][M] (its gradient w.r.t. x_)
    def _set_args(self, gps, Xs, mean_Xs, mean_grad):
        S = len(gps)
        P = len(gps[0]) if S else 0
        if S < 1 or P < 1 or any(len(row) != P for row in gps):
            raise BossError(BOSS_E_INVALID, "gps must be S rows of P posteriors")
        Xs = _f64(Xs, 2)
        du, M = Xs.shape
        dm = self.d_model if self.d_model is not None else du
        arr = (C.c_void_p * (P * S))()
        for s in range(S):
            for p in range(P):
                arr[p + P * s] = gps[s][p]._h
        ms = None if mean_Xs is None else np.ascontiguousarray(np.asarray(mean_Xs, dtype=np.float64).reshape(S, P, M))
        mg = None
        if mean_grad is not None:
            mg = np.ascontiguousarray(np.asarray(mean_grad, dtype=np.float64).reshape(S, P, dm, M).transpose(0, 1, 3, 2))
        return S, P, M, du, arr, Xs, ms, mg

    def predict(self, gps, Xs, mean_Xs=None):
        """(mu, var) [S, P, M] in user space (boss_warp_predict).  DomainError (.bad_index) at a model variance below -1e-8."""
        S, P, M, du, arr, Xs, ms, _ = self._set_args(gps, Xs, mean_Xs, None)
        mu, var = np.zeros((S, P, M)), np.zeros((S, P, M))
        bad = C.c_long(-1)
        try:
            _check(load_library().boss_warp_predict(self._h, P, S, arr, M, _dp(Xs), _dp(ms), _dp(mu), _dp(var), C.byref(bad)))
        except DomainError as e:
            e.bad_index = bad.value
            raise
        return mu, var

    def predict_grad(self, gps, Xs, mean_Xs=None, mean_grad=None):
        """(mu, var [S, P, M], dmu, dvar [S, P, d_user, M]) in user space (boss_warp_predict_grad)."""
        S, P, M, du, arr, Xs, ms, mg = self._set_args(gps, Xs, mean_Xs, mean_grad)
        mu, var = np.zeros((S, P, M)), np.zeros((S, P, M))
        dmu, dvar = np.zeros((S, P, M, du)), np.zeros((S, P, M, du))
        bad = C.c_long(-1)
        try:
            _check(load_library().boss_warp_predict_grad(self._h, P, S, arr, M, _dp(Xs), _dp(ms), _dp(mg), _dp(mu), _dp(var), _dp(dmu),
                                                         _dp(dvar), C.byref(bad)))
        except DomainError as e:
            e.bad_index = bad.value
            raise
        return mu, var, dmu.transpose(0, 1, 3, 2), dvar.transpose(0, 1, 3, 2)

    @staticmethod
    def _acq_args(fit_coefs, y_max, valid_mask):
        coefs = _f64(np.asarray(fit_coefs).reshape(-1), 1)
        ym = None if y_max is None else _f64(np.asarray(y_max).reshape(-1), 1)
        mask = None if valid_mask is None else np.ascontiguousarray(np.asarray(valid_mask, dtype=bool).astype(np.uint8))
        return coefs, ym, mask

    def acq_ei(self, gps, Xs, fit_coefs, y_max=None, best=None, valid_mask=None, mean_Xs=None, want_acq: bool = True):
        """EI × feasibility of the warped model over user-space candidates (boss_acq_ei_warp): (acq[M] or None, argmax, max)."""
        S, P, M, du, arr, Xs, ms, _ = self._set_args(gps, Xs, mean_Xs, None)
        coefs, ym, mask = self._acq_args(fit_coefs, y_max, valid_mask)
        acq = np.zeros(M) if want_acq else None
        am = C.c_long(-1)
        mx = C.c_double(0.0)
        _check(load_library().boss_acq_ei_warp(self._h, P, S, arr, M, _dp(Xs), _dp(ms), _dp(coefs), _dp(ym), 0 if best is None else 1,
                                               0.0 if best is None else float(best), _ucp(mask), _dp(acq), C.byref(am), C.byref(mx)))
        return acq, am.value, mx.value

    def acq_ei_grad(self, gps, Xs, fit_coefs, y_max=None, best=None, valid_mask=None, mean_Xs=None, mean_grad=None):
        """The same with its gradient w.r.t. the user-space candidates (boss_acq_ei_grad_warp): (acq[M], dacq[d_user, M])."""
        S, P, M, du, arr, Xs, ms, mg = self._set_args(gps, Xs, mean_Xs, mean_grad)
        coefs, ym, mask = self._acq_args(fit_coefs, y_max, valid_mask)
        acq = np.zeros(M)
        dacq = np.zeros((du, M), order="F")
        _check(load_library().boss_acq_ei_grad_warp(self._h, P, S, arr, M, _dp(Xs), _dp(ms), _dp(mg), _dp(coefs), _dp(ym),
                                                    0 if best is None else 1, 0.0 if best is None else float(best), _ucp(mask), _dp(acq),
                                                    _dp(dacq)))
        return acq, dacq

    def workgroup(self, stage: int, n: int, grad: bool, d_model: int = 0):
        """(waves per workgroup, dynamic LDS bytes) of stage 0 (the input warp) or 1 (the moments) for n candidates (tests)."""
        lib = load_library()
        lib.boss_debug_warp_block.restype = C.c_int
        lib.boss_debug_warp_block.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
        lds = C.c_int(0)
        return lib.boss_debug_warp_block(self._h, int(stage), 1 if grad else 0, int(n), int(d_model), C.byref(lds)), lds.value

    def close(self):
        if self._h:
            load_library().boss_warp_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------- several GPUs from one process (boss_multi_*)
def init() -> int:
    """boss_init: open every visible device and (when RCCL loads) a communicator on each; returns the device count."""
    n = C.c_int(0)
    _check(load_library().boss_init(C.byref(n)))
    return n.value


def comm_info():
    """(devices opened by init(), exchanges over RCCL?)"""
    n, r = C.c_int(0), C.c_int(0)
    _check(load_library().boss_comm_info(C.byref(n), C.byref(r)))
    return n.value, bool(r.value)


def shutdown():
    load_library().boss_shutdown()


def multi_update(replicas: Sequence[GP], lengthscale, amplitude, noise_std, mean_X=None) -> float:
    """The same hyper-parameters on the replicas of one posterior (replicas[g] on device g), factorised concurrently."""
    G = len(replicas)
    arr = (C.c_void_p * G)(*[r._h for r in replicas])
    lam = _f64(np.asarray(lengthscale).reshape(-1), 1)
    if lam.shape[0] != replicas[0].d:
        raise BossError(BOSS_E_INVALID, "length(lengthscales) must equal x_dim")
    m = None if mean_X is None else _f64(np.asarray(mean_X).reshape(-1), 1)
    out = C.c_double(0.0)
    _check(load_library().boss_multi_gp_update(G, arr, _dp(lam), float(amplitude), float(noise_std), _dp(m), C.byref(out)))
    for r in replicas:
        r.logpdf = out.value
    return out.value


def _acq_common(P, S, M, fit_coefs, y_max, valid_mask, mean_Xs):
    coefs = _f64(np.asarray(fit_coefs).reshape(-1), 1)
    ym = None if y_max is None else _f64(np.asarray(y_max).reshape(-1), 1)
    mask = None if valid_mask is None else np.ascontiguousarray(np.asarray(valid_mask, dtype=bool).astype(np.uint8))
    ms = None
    if mean_Xs is not None:
        a = np.asarray(mean_Xs, dtype=np.float64).reshape(S, P, M)
        ms = np.ascontiguousarray(a.transpose(0, 2, 1))       # index p + P*(j + M*s)
    return coefs, ym, mask, ms


def multi_acq_ei(replicas: Sequence[Sequence[Sequence[GP]]], Xs, fit_coefs, y_max=None, best=None, valid_mask=None,
                 mean_Xs=None, want_acq: bool = True):
    """boss_multi_acq_ei: candidates sharded over the devices.  replicas[g][s][p] = replica on device g of output p,
    hyper-parameter sample s.  Xs d×M (host); mean_Xs None or [S][P][M].  Returns (acq[M] or None, argmax, max)."""
    G, S, P = len(replicas), len(replicas[0]), len(replicas[0][0])
    Xs = _f64(Xs, 2)
    M = Xs.shape[1]
    arr = (C.c_void_p * (G * S * P))()
    for g in range(G):
        for s in range(S):
            for p in range(P):
                arr[p + P * (s + S * g)] = replicas[g][s][p]._h
    coefs, ym, mask, ms = _acq_common(P, S, M, fit_coefs, y_max, valid_mask, mean_Xs)
    acq = np.zeros(M) if want_acq else None
    am, mx = C.c_long(-1), C.c_double(0.0)
    _check(load_library().boss_multi_acq_ei(G, P, S, arr, M, _dp(Xs), _dp(ms), _dp(coefs), _dp(ym), 0 if best is None else 1,
                                            0.0 if best is None else float(best), _ucp(mask), _dp(acq), C.byref(am), C.byref(mx)))
    return acq, am.value, mx.value


class MultiCandidates:
    """boss_multi_cand_create: candidates resident on G devices (shard g = the g-th balanced contiguous range of the columns)."""

    def __init__(self, Xs, G: int):
        Xs = _f64(Xs, 2)
        self.d, self.M, self.G = Xs.shape[0], Xs.shape[1], int(G)
        self._h = C.c_void_p()
        _check(load_library().boss_multi_cand_create(self.G, self.d, self.M, _dp(Xs), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            load_library().boss_multi_cand_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def multi_acq_ei_cand(replicas: Sequence[Sequence[Sequence[GP]]], cand: MultiCandidates, fit_coefs, y_max=None, best=None,
                      valid_mask=None, mean_Xs=None, want_acq: bool = True):
    """boss_multi_acq_ei_cand: multi_acq_ei on resident candidate shards.  Returns (acq[M] or None, argmax, max)."""
    G, S, P = len(replicas), len(replicas[0]), len(replicas[0][0])
    M = cand.M
    arr = (C.c_void_p * (G * S * P))()
    for g in range(G):
        for s in range(S):
            for p in range(P):
                arr[p + P * (s + S * g)] = replicas[g][s][p]._h
    coefs, ym, mask, ms = _acq_common(P, S, M, fit_coefs, y_max, valid_mask, mean_Xs)
    acq = np.zeros(M) if want_acq else None
    am, mx = C.c_long(-1), C.c_double(0.0)
    _check(load_library().boss_multi_acq_ei_cand(G, P, S, arr, cand._h, _dp(ms), _dp(coefs), _dp(ym), 0 if best is None else 1,
                                                 0.0 if best is None else float(best), _ucp(mask), _dp(acq), C.byref(am), C.byref(mx)))
    return acq, am.value, mx.value


def _multi_handles(fn_name, gps, Xs, fit_coefs, y_max, best, valid_mask, mean_Xs, want_acq):
    S, P = len(gps), len(gps[0])
    Xs = _f64(Xs, 2)
    M = Xs.shape[1]
    arr = (C.c_void_p * (P * S))()
    for s in range(S):
        for p in range(P):
            arr[p + P * s] = gps[s][p]._h
    coefs, ym, mask, ms = _acq_common(P, S, M, fit_coefs, y_max, valid_mask, mean_Xs)
    acq = np.zeros(M) if want_acq else None
    am, mx = C.c_long(-1), C.c_double(0.0)
    _check(getattr(load_library(), fn_name)(P, S, arr, M, _dp(Xs), _dp(ms), _dp(coefs), _dp(ym), 0 if best is None else 1,
                                            0.0 if best is None else float(best), _ucp(mask), _dp(acq), C.byref(am), C.byref(mx)))
    return acq, am.value, mx.value


def multi_acq_ei_outputs(gps: Sequence[Sequence[GP]], Xs, fit_coefs, y_max=None, best=None, valid_mask=None, mean_Xs=None,
                         want_acq: bool = True):
    """boss_multi_acq_ei_outputs: gps[s][p] may live on any device (outputs sharded one per GPU)."""
    return _multi_handles("boss_multi_acq_ei_outputs", gps, Xs, fit_coefs, y_max, best, valid_mask, mean_Xs, want_acq)


def multi_acq_ei_samples(gps: Sequence[Sequence[GP]], Xs, fit_coefs, y_max=None, best=None, valid_mask=None, mean_Xs=None,
                         want_acq: bool = True):
    """boss_multi_acq_ei_samples: all outputs of sample s on one device, different samples on different devices."""
    return _multi_handles("boss_multi_acq_ei_samples", gps, Xs, fit_coefs, y_max, best, valid_mask, mean_Xs, want_acq)


def multi_loglike_batch(G: int, X, y, kernel, lengthscales, amplitudes, noise_stds, mean_X=None, discrete=None):
    """boss_multi_loglike_batch: the S hyper-parameter sets split over devices 0..G-1.  Returns (ll[S], status[S])."""
    X = _f64(X, 2)
    y = _f64(np.asarray(y).reshape(-1), 1)
    lam = _f64(lengthscales, 2)
    d, N = X.shape
    S = lam.shape[1]
    if lam.shape[0] != d:
        raise BossError(BOSS_E_INVALID, "lengthscales must be d×S")
    amp = _f64(np.asarray(amplitudes).reshape(-1), 1)
    sig = _f64(np.asarray(noise_stds).reshape(-1), 1)
    stride, m = 0, None
    if mean_X is not None:
        m = np.asarray(mean_X, dtype=np.float64)
        if m.ndim == 2:
            m, stride = np.ascontiguousarray(m), N
        else:
            m = np.ascontiguousarray(m.reshape(-1))
    disc = None if discrete is None else np.ascontiguousarray(np.asarray(discrete, dtype=bool).astype(np.uint8))
    ll = np.zeros(S)
    st = np.zeros(S, dtype=np.int32)
    _check(load_library().boss_multi_loglike_batch(G, _kernel_id(kernel), d, N, _dp(X), _dp(y), _dp(m), stride, _ucp(disc), S,
                                                   _dp(lam), _dp(amp), _dp(sig), _dp(ll), st.ctypes.data_as(C.POINTER(C.c_int))))
    return ll, st


def bench_mfma_f64(device: int = 0, iters: int = 20000) -> float:
    out = C.c_double(0.0)
    _check(load_library().boss_bench_mfma_f64(device, iters, C.byref(out)))
    return out.value


def prof_enable(device: int, on: bool):
    _check(load_library().boss_prof_enable(device, 1 if on else 0))


def prof_reset(device: int):
    _check(load_library().boss_prof_reset(device))


def prof_get(device: int, kernel_class: str):
    ms = C.c_double(0.0)
    n = C.c_long(0)
    _check(load_library().boss_prof_get(device, kernel_class.encode(), C.byref(ms), C.byref(n)))
    return ms.value, n.value


def _update_path(g: GP):
    """(chained, trail_mode, fell_back) of the handle's last completed update (boss_debug_update_path; tests): whether it ran
    under the resident panel chain, the trailing schedule it used there (4: the deferred schedule's work table; -1: no chain),
    and whether it was repeated on a simpler schedule."""
    lib = load_library()
    fn = lib.boss_debug_update_path
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    ch, tm, fb = C.c_int(0), C.c_int(0), C.c_int(0)
    _check(fn(g._h, C.byref(ch), C.byref(tm), C.byref(fb)))
    return ch.value, tm.value, fb.value


def _append_path(g: GP) -> int:
    """How the handle's last append ran (boss_debug_append_path; tests): 0 no append yet, 1 block rows, 2 full re-factorisation on
    the device, 3 rank-one on resident inverses."""
    fn = load_library().boss_debug_append_path
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    out = C.c_int(-1)
    _check(fn(g._h, C.byref(out)))
    return out.value


def _fallbacks(device: int = 0):
    """(updates repeated on a simpler schedule so far in this process, whether the resident chain is off on `device`)
    (boss_debug_fallbacks; tests)."""
    lib = load_library()
    fn = lib.boss_debug_fallbacks
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.POINTER(C.c_long), C.POINTER(C.c_int)]
    n, off = C.c_long(0), C.c_int(0)
    _check(fn(device, C.byref(n), C.byref(off)))
    return n.value, off.value


def _set_launches(device: int = 0):
    """(all, on precomputed K*) launches of the one-launch set prediction on the device so far (boss_debug_set_launches; tests)."""
    lib = load_library()
    fn = lib.boss_debug_set_launches
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.POINTER(C.c_long), C.POINTER(C.c_long)]
    a, b = C.c_long(0), C.c_long(0)
    fn(device, C.byref(a), C.byref(b))
    return a.value, b.value


def _set_grad_launches(device: int = 0):
    """Launches of the set adjoint substitution (boss_acq_ei_grad_set's set path) on the device so far
    (boss_debug_set_grad_launches; tests)."""
    lib = load_library()
    fn = lib.boss_debug_set_grad_launches
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.POINTER(C.c_long)]
    a = C.c_long(0)
    fn(device, C.byref(a))
    return a.value


def _acq_path(device: int = 0):
    """What the last arg-max-only boss_acq_ei on `device` did (boss_debug_acq_path; tests): (path, round-1 count, round-2 count,
    head blocks s, whether a = L⁻ᵀz was rebuilt); path 0: full kernel, 1: pruned, 2: fallback after an attempt, 3: skipped by the
    back-off."""
    fn = load_library().boss_debug_acq_path
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.POINTER(C.c_int)]
    out = (C.c_int * 5)()
    _check(fn(device, out))
    return tuple(out)


def _acq_prune_set(device: int = 0, min_tiles: int = -1, K: int = -1, s: int = -1, cap: int = -1, slack: Optional[float] = None):
    """Settings of the arg-max-only acquisition path (boss_debug_acq_prune_set / boss_debug_acq_prune_slack; tests): candidate tiles
    above which it is tried, round-1 size, head blocks, round-2 cap, scale of the bound's slacks.  -1 / None keeps a value, anything
    below -1 restores its default."""
    lib = load_library()
    fn = lib.boss_debug_acq_prune_set
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * 5
    _check(fn(device, int(min_tiles), int(K), int(s), int(cap)))
    if slack is not None:
        fs = lib.boss_debug_acq_prune_slack
        fs.restype = C.c_int
        fs.argtypes = [C.c_int, C.c_double]
        _check(fs(device, float(slack)))


def _acq_prune_bounds(M: int, device: int = 0):
    """(μ_a, σ²_s, ub) of the last pruned attempt over M candidates on `device` (boss_debug_acq_prune_bounds; measurements)."""
    fn = load_library().boss_debug_acq_prune_bounds
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    mua, vs, ub = np.zeros(M), np.zeros(M), np.zeros(M)
    _check(fn(device, int(M), mua.ctypes.data, vs.ctypes.data, ub.ctypes.data))
    return mua, vs, ub


def _acq_counters(g: GP):
    """(resident inverse factors exist, few-candidates call count of the handle, device allocations of the process, kernels the
    arg-max-only path enqueued on the handle's device) (boss_debug_acq_counters; tests)."""
    fn = load_library().boss_debug_acq_counters
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_long)]
    out = (C.c_long * 4)()
    _check(fn(g._h, out))
    return tuple(out)
