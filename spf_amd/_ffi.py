"""ctypes binding of the C ABI in include/spf_hip.h.

``Engine`` wraps one ``spf_ctx`` (one GPU).  Host-array methods take / return numpy arrays and
go through the ``*_batch`` entry points; ``*_dev`` methods take raw device pointers (e.g.
``torch.Tensor.data_ptr()``) and a stream handle and are asynchronous.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from .params import Params, DEFAULT_128

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class SpfError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"spf_hip status {status}: {msg}")
        self.status = status


class _CParams(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in (
        "lwe_dimension", "polynomial_degree", "glwe_size", "pbs_radix_log", "pbs_radix_count",
        "cbs_radix_log", "cbs_radix_count", "ks_radix_log", "ks_radix_count", "tr_radix_log",
        "tr_radix_count", "ss_radix_log", "ss_radix_count")]


# spf_value_kind of the LWE ciphertexts, and the number of weight slots of a context (include/spf_hip.h)
VAL_LWE0, VAL_LWE1 = 0, 1
VAL_GLWE1 = 2   # (the other leaf kind of Engine.lwe_ring_pack)
LWE_LINEAR_SLOTS = 64
# the limits of the plaintext polynomial weights over GLWE ciphertexts (spf_glwe_poly_limits)
GLWE_POLY_SLOTS, GLWE_POLY_MAX_ROWS, GLWE_POLY_MAX_TERMS = 64, 4096, 1 << 24
# the key slots of the GLWE keyswitch (spf_glwe_ksk_limits)
GLWE_KSK_SLOTS = 16


def lib_path() -> str:
    # SPF_HIP_LIBRARY lets experiments (e.g. A/B builds of the kept knobs, tools/ab_build.sh) swap the library
    return os.environ.get("SPF_HIP_LIBRARY") or os.path.join(_HERE, "lib", "libspf_hip.so")


# every symbol include/spf_hip.h declares: (name, restype, argtypes)
_P, _SZ, _U32, _U64, _I = C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64, C.c_int
SYMBOLS = [
    ("spf_default_params", None, [C.POINTER(_CParams)]),
    ("spf_create", _I, [C.POINTER(_CParams), _I, C.POINTER(_P)]),
    ("spf_destroy", None, [_P]),
    ("spf_last_error", C.c_char_p, [_P]),
    ("spf_load_bootstrap_key", _I, [_P, _P, _SZ]),
    ("spf_load_keyswitch_key", _I, [_P, _P, _SZ]),
    ("spf_load_automorphism_key", _I, [_P, _P, _SZ]),
    ("spf_load_scheme_switch_key", _I, [_P, _P, _SZ]),
    ("spf_poly_fft_dev", _I, [_P, _P, _SZ, _P, _P]),
    ("spf_poly_fft_batch", _I, [_P, _SZ, _P, _P]),
    ("spf_load_bootstrap_key_std", _I, [_P, _P, _SZ]),
    ("spf_load_automorphism_key_std", _I, [_P, _P, _SZ]),
    ("spf_load_scheme_switch_key_std", _I, [_P, _P, _SZ]),
    ("spf_load_public_functional_keyswitch_key_std", _I, [_P, _P, _SZ, _SZ, _U32, _U32]),
    ("spf_load_private_functional_keyswitch_keys_std", _I, [_P, _P, _SZ, _SZ, _SZ, _SZ, _U32, _U32]),
    ("spf_key_blob", _I, [_P, _I, C.POINTER(_P), C.POINTER(_SZ)]),
    ("spf_key_blob_commit", _I, [_P, _I]),
    ("spf_keyswitch_lwe_l1_lwe_l0_batch", _I, [_P, _SZ, _P, _P]),
    ("spf_generalized_pbs_batch", _I, [_P, _SZ, _P, _P, _SZ, _U32, _U32, _U64, _P]),
    ("spf_pbs_univariate_batch", _I, [_P, _SZ, _P, _P, _SZ, _P]),
    ("spf_pbs_bivariate_batch", _I, [_P, _SZ, _P, _P, _P, _SZ, _U32, _P]),
    ("spf_circuit_bootstrap_pbs_batch", _I, [_P, _SZ, _P, _P]),
    ("spf_circuit_bootstrap_batch", _I, [_P, _SZ, _P, _P]),
    ("spf_mod_switch_trace_and_rotate_batch", _I, [_P, _SZ, _P, _P]),
    ("spf_scheme_switch_batch", _I, [_P, _SZ, _P, _P]),
    ("spf_sample_extract_l1_batch", _I, [_P, _SZ, _P, _SZ, _P]),
    ("spf_glwe_not_batch", _I, [_P, _SZ, _P, _P]),
    ("spf_glwe_xor_batch", _I, [_P, _SZ, _P, _P, _P]),
    ("spf_glwe_mul_xn_batch", _I, [_P, _SZ, _P, _SZ, _P]),
    ("spf_glwe_not_dev", _I, [_P, _P, _SZ, _P, _P]),
    ("spf_glwe_xor_dev", _I, [_P, _P, _SZ, _P, _P, _P]),
    ("spf_glwe_mul_xn_dev", _I, [_P, _P, _SZ, _P, _SZ, _P]),
    ("spf_cmux_batch", _I, [_P, _SZ, _P, _P, _P, _P]),
    ("spf_glev_cmux_batch", _I, [_P, _SZ, _P, _P, _P, _P]),
    ("spf_multiply_glwe_ggsw_batch", _I, [_P, _SZ, _P, _P, _P]),
    ("spf_glev_cmux_dev", _I, [_P, _P, _SZ, _P, _P, _P, _P]),
    ("spf_multiply_glwe_ggsw_dev", _I, [_P, _P, _SZ, _P, _P, _P]),
    ("spf_glwe_pack_dev", _I, [_P, _P, _SZ, _SZ, _P, _P]),
    ("spf_glwe_unpack_l1_dev", _I, [_P, _P, _SZ, _SZ, _P, _P]),
    ("spf_unpack_circuit_bootstrap_dev", _I, [_P, _P, _SZ, _SZ, _P, _P]),
    ("spf_gate_bootstrap_batch", _I, [_P, _SZ, _P, _P]),
    ("spf_keyswitch_circuit_bootstrap_batch", _I, [_P, _SZ, _P, _P]),
    ("spf_glwe_pack_batch", _I, [_P, _SZ, _SZ, _P, _P]),
    ("spf_glwe_unpack_l1_batch", _I, [_P, _SZ, _SZ, _P, _P]),
    ("spf_unpack_circuit_bootstrap_batch", _I, [_P, _SZ, _SZ, _P, _P]),
    ("spf_blind_rotation_batch", _I, [_P, _SZ, _SZ, _SZ, _P, _P, _P]),
    ("spf_blind_rotation_dev", _I, [_P, _P, _SZ, _SZ, _SZ, _P, _P, _P]),
    ("spf_public_functional_keyswitch_batch", _I, [_P, _SZ, _SZ, _P, _P]),
    ("spf_public_functional_keyswitch_enqueue", _I, [_P, _P, _SZ, _SZ, _P, _P]),
    ("spf_private_functional_keyswitch_batch", _I, [_P, _SZ, _SZ, _P, _P]),
    ("spf_private_functional_keyswitch_enqueue", _I, [_P, _P, _SZ, _SZ, _P, _P]),
    ("spf_apply_pfks_on_ggsw_components_batch", _I, [_P, _SZ, _P, _P]),
    ("spf_apply_pfks_on_ggsw_components_enqueue", _I, [_P, _P, _SZ, _P, _P]),
    ("spf_circuit_bootstrap_via_pfks_batch", _I, [_P, _SZ, _P, _P]),
    ("spf_circuit_bootstrap_via_pfks_enqueue", _I, [_P, _P, _SZ, _P, _P]),
    ("spf_load_lwe_linear_weights", _I, [_P, _U32, _SZ, _SZ, _P, _P]),
    ("spf_lwe_linear_batch", _I, [_P, _U32, _I, _SZ, _P, _P]),
    ("spf_lwe_linear_enqueue", _I, [_P, _P, _U32, _I, _SZ, _P, _P]),
    ("spf_last_lwe_linear_kernel", C.c_char_p, [_P]),
    ("spf_lwe_linear_slot_shape", _I, [_P, _U32, C.POINTER(_SZ), C.POINTER(_SZ), C.POINTER(C.c_int)]),
    ("spf_load_glwe_poly_weights", _I, [_P, _U32, _SZ, _SZ, _P, _P, _P, _P]),
    ("spf_glwe_poly_linear_batch", _I, [_P, _U32, _SZ, _P, _P]),
    ("spf_glwe_poly_linear_enqueue", _I, [_P, _P, _U32, _SZ, _P, _P]),
    ("spf_glwe_poly_slot_shape", _I, [_P, _U32, C.POINTER(_SZ), C.POINTER(_SZ), C.POINTER(_SZ), C.POINTER(C.c_int)]),
    ("spf_last_glwe_poly_kernel", C.c_char_p, [_P]),
    ("spf_load_glwe_keyswitch_key_std", _I, [_P, _U32, _P, _SZ, _U32, _U32]),
    ("spf_glwe_keyswitch_slot_shape", _I, [_P, _U32, C.POINTER(_U32), C.POINTER(_U32)]),
    ("spf_glwe_keyswitch_batch", _I, [_P, _U32, _SZ, _P, _P]),
    ("spf_glwe_keyswitch_enqueue", _I, [_P, _P, _U32, _SZ, _P, _P]),
    ("spf_glwe_automorphism_batch", _I, [_P, _U32, _SZ, _P, _P]),
    ("spf_glwe_automorphism_enqueue", _I, [_P, _P, _U32, _SZ, _P, _P]),
    ("spf_glwe_trace_batch", _I, [_P, _SZ, _P, _P]),
    ("spf_glwe_trace_enqueue", _I, [_P, _P, _SZ, _P, _P]),
    ("spf_last_glwe_keyswitch_kernel", C.c_char_p, [_P]),
    ("spf_lwe_ring_pack_batch", _I, [_P, _I, _SZ, _SZ, _P, _P]),
    ("spf_lwe_ring_pack_scratch_words", _I, [_P, _SZ, _SZ, C.POINTER(_SZ)]),
    ("spf_lwe_ring_pack_enqueue", _I, [_P, _P, _I, _SZ, _SZ, _P, _P, _SZ, _P]),
    ("spf_last_lwe_ring_pack_kernel", C.c_char_p, [_P]),
    # the per-item forms: (ctx, [stream,] B, in, HOST array of B parameters, out)
    ("spf_sample_extract_l1_each_batch", _I, [_P, _SZ, _P, _P, _P]),
    ("spf_sample_extract_l1_each_devptr", _I, [_P, _P, _SZ, _P, _P, _P]),
    ("spf_glwe_mul_xn_each_batch", _I, [_P, _SZ, _P, _P, _P]),
    ("spf_glwe_mul_xn_each_devptr", _I, [_P, _P, _SZ, _P, _P, _P]),
    ("spf_glwe_keyswitch_each_batch", _I, [_P, _SZ, _P, _P, _P]),
    ("spf_glwe_keyswitch_each_devptr", _I, [_P, _P, _SZ, _P, _P, _P]),
    ("spf_glwe_automorphism_each_batch", _I, [_P, _SZ, _P, _P, _P]),
    ("spf_glwe_automorphism_each_devptr", _I, [_P, _P, _SZ, _P, _P, _P]),
    ("spf_keyswitch_lwe_l1_lwe_l0_dev", _I, [_P, _P, _SZ, _P, _P]),
    ("spf_generalized_pbs_dev", _I, [_P, _P, _SZ, _P, _P, _SZ, _U32, _U32, _U64, _P]),
    ("spf_pbs_univariate_dev", _I, [_P, _P, _SZ, _P, _P, _SZ, _P]),
    ("spf_pbs_bivariate_dev", _I, [_P, _P, _SZ, _P, _P, _P, _SZ, _U32, _P]),
    ("spf_circuit_bootstrap_pbs_dev", _I, [_P, _P, _SZ, _P, _P]),
    ("spf_circuit_bootstrap_dev", _I, [_P, _P, _SZ, _P, _P]),
    ("spf_mod_switch_trace_and_rotate_dev", _I, [_P, _P, _SZ, _P, _P]),
    ("spf_scheme_switch_dev", _I, [_P, _P, _SZ, _P, _P]),
    ("spf_sample_extract_l1_dev", _I, [_P, _P, _SZ, _P, _SZ, _P]),
    ("spf_cmux_dev", _I, [_P, _P, _SZ, _P, _P, _P, _P]),
    ("spf_pool_create", _I, [_P, _SZ, _U32, C.POINTER(_P)]),
    ("spf_pool_destroy", None, [_P]),
    ("spf_pool_submit_keyswitch", _I, [_P, _P, _P, C.POINTER(_U64)]),
    ("spf_pool_submit_circuit_bootstrap", _I, [_P, _P, _P, C.POINTER(_U64)]),
    ("spf_pool_submit_keyswitch_circuit_bootstrap", _I, [_P, _P, _P, C.POINTER(_U64)]),
    ("spf_pool_submit_cmux", _I, [_P, _P, _P, _P, _P, C.POINTER(_U64)]),
    ("spf_pool_submit_sample_extract", _I, [_P, _P, _SZ, _P, C.POINTER(_U64)]),
    ("spf_pool_submit_not", _I, [_P, _P, _P, C.POINTER(_U64)]),
    ("spf_pool_submit_glwe_add", _I, [_P, _P, _P, _P, C.POINTER(_U64)]),
    ("spf_pool_submit_mul_xn", _I, [_P, _P, _SZ, _P, C.POINTER(_U64)]),
    ("spf_pool_submit_multiply_ggsw_glwe", _I, [_P, _P, _P, _P, C.POINTER(_U64)]),
    ("spf_pool_submit_glev_cmux", _I, [_P, _P, _P, _P, _P, C.POINTER(_U64)]),
    ("spf_pool_submit_scheme_switch", _I, [_P, _P, _P, C.POINTER(_U64)]),
    ("spf_pool_submit_glwe_keyswitch", _I, [_P, _U32, _P, _P, C.POINTER(_U64)]),
    ("spf_pool_submit_glwe_automorphism", _I, [_P, _U32, _P, _P, C.POINTER(_U64)]),
    ("spf_pool_submit_glwe_trace", _I, [_P, _P, _P, C.POINTER(_U64)]),
    ("spf_pool_wait", _I, [_P, _U64]),
    ("spf_pool_set_max_inflight", _I, [_P, _SZ]),
    ("spf_pool_set_mixed_parameters", _I, [_P, C.c_int]),
    ("spf_pool_stats", _I, [_P, C.POINTER(_U64), C.POINTER(_U64)]),
    ("spf_graph_create", _I, [_P, C.POINTER(_P)]),
    ("spf_graph_destroy", None, [_P]),
    ("spf_graph_add_input", _I, [_P, _I, _P, C.POINTER(_U32)]),
    ("spf_graph_add_trivial", _I, [_P, _I, _U64, C.POINTER(_U32)]),
    ("spf_graph_add_op", _I, [_P, _I, C.POINTER(_U32), _SZ, _U64, C.POINTER(_U32)]),
    ("spf_graph_add_unpack", _I, [_P, _U32, _SZ, C.POINTER(_U32)]),
    ("spf_graph_add_pack", _I, [_P, C.POINTER(_U32), _SZ, C.POINTER(_U32)]),
    ("spf_graph_add_blind_rotation", _I, [_P, _U32, C.POINTER(_U32), _SZ, _SZ, C.POINTER(_U32)]),
    ("spf_graph_add_public_functional_keyswitch", _I, [_P, C.POINTER(_U32), _SZ, C.POINTER(_U32)]),
    ("spf_graph_add_lwe_linear", _I, [_P, _U32, C.POINTER(_U32), _SZ, _SZ, C.POINTER(_U32)]),
    ("spf_graph_add_glwe_poly_linear", _I, [_P, _U32, C.POINTER(_U32), _SZ, _SZ, C.POINTER(_U32)]),
    ("spf_graph_add_glwe_keyswitch", _I, [_P, _U32, _U32, C.POINTER(_U32)]),
    ("spf_graph_add_glwe_automorphism", _I, [_P, _U32, _U32, C.POINTER(_U32)]),
    ("spf_graph_add_glwe_trace", _I, [_P, _U32, C.POINTER(_U32)]),
    ("spf_graph_add_output", _I, [_P, _U32, _P]),
    ("spf_graph_run", _I, [_P]),
    ("spf_graph_stats", _I, [_P, C.POINTER(_U32), C.POINTER(_U32), C.POINTER(_U32)]),
    ("spf_cmux_scattered_dev", _I, [_P, _P, _SZ, _P]),
    ("spf_gather_rows_dev", _I, [_P, _P, _SZ, _SZ, _P, _P]),
    ("spf_set_timing", _I, [_P, _I]),
    ("spf_last_kernel_ms", _I, [_P, C.c_char_p, C.POINTER(C.c_double), C.POINTER(_I)]),
    ("spf_last_blind_rotate_kernel", C.c_char_p, [_P]),
    ("spf_last_cmux_kernel", C.c_char_p, [_P]),
    ("spf_last_public_functional_keyswitch_kernel", C.c_char_p, [_P]),
    ("spf_last_private_functional_keyswitch_kernel", C.c_char_p, [_P]),
    ("spf_last_keyswitch_kernel", C.c_char_p, [_P]),
    ("spf_device_alloc", _I, [_P, _SZ, C.POINTER(_P)]),
    ("spf_device_free", _I, [_P, _P]),
    ("spf_device_upload", _I, [_P, _P, _P, _SZ]),
    ("spf_device_download", _I, [_P, _P, _P, _P, _SZ]),
    ("spf_l1ggsw_constant", _I, [_P, _I, _P]),
    ("spf_generate_lut", _I, [C.POINTER(_CParams), _P, _SZ, _U32, _P]),
    ("spf_generate_bivariate_lut", _I, [C.POINTER(_CParams), _P, _U32, _U32, _P]),
    ("spf_load_compute_key_bincode", _I, [_P, _P, _SZ]),
    ("spf_load_compute_key_nonfft_bincode", _I, [_P, _P, _SZ]),
    ("spf_ciphertext_words", _SZ, [C.POINTER(_CParams), _I]),
    ("spf_ciphertext_from_bincode", _I, [C.POINTER(_CParams), _I, _P, _SZ, _P]),
    ("spf_ciphertext_to_bincode", _I, [C.POINTER(_CParams), _I, _P, _P, _SZ, C.POINTER(_SZ)]),
    ("spf_version", C.c_char_p, []),
    ("spf_live_objects", _I, [C.POINTER(_U64 * 5)]),
    # device groups (one host process, every GPU of the node)
    ("spf_group_create", _I, [C.POINTER(_CParams), C.POINTER(_I), _I, C.POINTER(_P)]),
    ("spf_group_destroy", None, [_P]),
    ("spf_group_size", _I, [_P]),
    ("spf_group_ctx", _P, [_P, _I]),
    ("spf_group_last_error", C.c_char_p, [_P]),
    ("spf_group_load_bootstrap_key", _I, [_P, _P, _SZ]),
    ("spf_group_load_keyswitch_key", _I, [_P, _P, _SZ]),
    ("spf_group_load_automorphism_key", _I, [_P, _P, _SZ]),
    ("spf_group_load_scheme_switch_key", _I, [_P, _P, _SZ]),
    ("spf_group_load_compute_key_bincode", _I, [_P, _P, _SZ]),
    ("spf_group_load_bootstrap_key_std", _I, [_P, _P, _SZ]),
    ("spf_group_load_automorphism_key_std", _I, [_P, _P, _SZ]),
    ("spf_group_load_scheme_switch_key_std", _I, [_P, _P, _SZ]),
    ("spf_group_load_public_functional_keyswitch_key_std", _I, [_P, _P, _SZ, _SZ, _U32, _U32]),
    ("spf_group_load_private_functional_keyswitch_keys_std", _I, [_P, _P, _SZ, _SZ, _SZ, _SZ, _U32, _U32]),
    ("spf_group_load_compute_key_nonfft_bincode", _I, [_P, _P, _SZ]),
    ("spf_group_replicate_keys", _I, [_P]),
    ("spf_group_replication_stats", _I, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_SZ), C.POINTER(_I),
                                         C.POINTER(C.c_char_p)]),
    ("spf_group_set_member_enabled", _I, [_P, _I, _I]),
    ("spf_group_members_in_rotation", _I, [_P]),
    ("spf_group_debug_fail_next", _I, [_P, _I, _I]),
    ("spf_group_keyswitch_lwe_l1_lwe_l0_batch", _I, [_P, _SZ, _P, _P]),
    ("spf_group_generalized_pbs_batch", _I, [_P, _SZ, _P, _P, _SZ, _U32, _U32, _U64, _P]),
    ("spf_group_pbs_univariate_batch", _I, [_P, _SZ, _P, _P, _SZ, _P]),
    ("spf_group_pbs_bivariate_batch", _I, [_P, _SZ, _P, _P, _P, _SZ, _U32, _P]),
    ("spf_group_circuit_bootstrap_pbs_batch", _I, [_P, _SZ, _P, _P]),
    ("spf_group_circuit_bootstrap_batch", _I, [_P, _SZ, _P, _P]),
    ("spf_group_mod_switch_trace_and_rotate_batch", _I, [_P, _SZ, _P, _P]),
    ("spf_group_scheme_switch_batch", _I, [_P, _SZ, _P, _P]),
    ("spf_group_sample_extract_l1_batch", _I, [_P, _SZ, _P, _SZ, _P]),
    ("spf_group_glwe_not_batch", _I, [_P, _SZ, _P, _P]),
    ("spf_group_glwe_xor_batch", _I, [_P, _SZ, _P, _P, _P]),
    ("spf_group_glwe_mul_xn_batch", _I, [_P, _SZ, _P, _SZ, _P]),
    ("spf_group_cmux_batch", _I, [_P, _SZ, _P, _P, _P, _P]),
    ("spf_group_glev_cmux_batch", _I, [_P, _SZ, _P, _P, _P, _P]),
    ("spf_group_multiply_glwe_ggsw_batch", _I, [_P, _SZ, _P, _P, _P]),
    ("spf_group_gate_bootstrap_batch", _I, [_P, _SZ, _P, _P]),
    ("spf_group_keyswitch_circuit_bootstrap_batch", _I, [_P, _SZ, _P, _P]),
    ("spf_group_glwe_pack_batch", _I, [_P, _SZ, _SZ, _P, _P]),
    ("spf_group_glwe_unpack_l1_batch", _I, [_P, _SZ, _SZ, _P, _P]),
    ("spf_group_unpack_circuit_bootstrap_batch", _I, [_P, _SZ, _SZ, _P, _P]),
    ("spf_group_blind_rotation_batch", _I, [_P, _SZ, _SZ, _SZ, _P, _P, _P]),
    ("spf_group_public_functional_keyswitch_batch", _I, [_P, _SZ, _SZ, _P, _P]),
    ("spf_group_private_functional_keyswitch_batch", _I, [_P, _SZ, _SZ, _P, _P]),
    ("spf_group_circuit_bootstrap_via_pfks_batch", _I, [_P, _SZ, _P, _P]),
    ("spf_group_load_lwe_linear_weights", _I, [_P, _U32, _SZ, _SZ, _P, _P]),
    ("spf_group_lwe_linear_batch", _I, [_P, _U32, _I, _SZ, _P, _P]),
    ("spf_group_load_glwe_poly_weights", _I, [_P, _U32, _SZ, _SZ, _P, _P, _P, _P]),
    ("spf_group_glwe_poly_linear_batch", _I, [_P, _U32, _SZ, _P, _P]),
    ("spf_group_load_glwe_keyswitch_key_std", _I, [_P, _U32, _P, _SZ, _U32, _U32]),
    ("spf_group_glwe_keyswitch_batch", _I, [_P, _U32, _SZ, _P, _P]),
    ("spf_group_glwe_automorphism_batch", _I, [_P, _U32, _SZ, _P, _P]),
    ("spf_group_sample_extract_l1_each_batch", _I, [_P, _SZ, _P, _P, _P]),
    ("spf_group_glwe_mul_xn_each_batch", _I, [_P, _SZ, _P, _P, _P]),
    ("spf_group_glwe_keyswitch_each_batch", _I, [_P, _SZ, _P, _P, _P]),
    ("spf_group_glwe_automorphism_each_batch", _I, [_P, _SZ, _P, _P, _P]),
    ("spf_group_glwe_trace_batch", _I, [_P, _SZ, _P, _P]),
    ("spf_group_lwe_ring_pack_batch", _I, [_P, _I, _SZ, _SZ, _P, _P]),
    ("spf_group_l1ggsw_constant", _I, [_P, _I, _P]),
    ("spf_pool_create_group", _I, [_P, _SZ, _U32, C.POINTER(_P)]),
    ("spf_group_graph_create", _I, [_P, C.POINTER(_P)]),
    ("spf_group_run_graphs", _I, [_P, C.POINTER(_P), _SZ]),
    ("spf_graph_member", _I, [_P]),
    # device-resident values and the pool's submits by handle
    ("spf_pool_counters_get", _I, [_P, C.POINTER(_U64 * 11)]),
    ("spf_value_upload", _I, [_P, _I, _I, _P, C.POINTER(_P)]),
    ("spf_value_upload_batch", _I, [_P, _I, _I, _SZ, _P, C.POINTER(_P)]),
    ("spf_value_download_batch", _I, [_SZ, C.POINTER(_P), _P]),
    ("spf_value_trivial", _I, [_P, _I, _I, _U64, C.POINTER(_P)]),
    ("spf_value_download", _I, [_P, _P]),
    ("spf_value_wait", _I, [_P]),
    ("spf_pool_flush", _I, [_P]),
    ("spf_value_retain", _I, [_P]),
    ("spf_value_release", None, [_P]),
    ("spf_value_info", _I, [_P, C.POINTER(_I), C.POINTER(_SZ), C.POINTER(_I), C.POINTER(_I)]),
    ("spf_value_device_ptr", _I, [_P, C.POINTER(_P)]),
    ("spf_value_copy_to_member", _I, [_P, _P, _I, C.POINTER(_P)]),
    ("spf_pool_value_stats", _I, [_P, C.POINTER(_SZ), C.POINTER(_SZ), C.POINTER(_SZ)]),
    ("spf_pool_trim", _I, [_P]),
    ("spf_pool_submit_keyswitch_v", _I, [_P, _P, C.POINTER(_P), C.POINTER(_U64)]),
    ("spf_pool_submit_circuit_bootstrap_v", _I, [_P, _P, C.POINTER(_P), C.POINTER(_U64)]),
    ("spf_pool_submit_keyswitch_circuit_bootstrap_v", _I, [_P, _P, C.POINTER(_P), C.POINTER(_U64)]),
    ("spf_pool_submit_cmux_v", _I, [_P, _P, _P, _P, C.POINTER(_P), C.POINTER(_U64)]),
    ("spf_pool_submit_sample_extract_v", _I, [_P, _P, _SZ, C.POINTER(_P), C.POINTER(_U64)]),
    ("spf_pool_submit_not_v", _I, [_P, _P, C.POINTER(_P), C.POINTER(_U64)]),
    ("spf_pool_submit_glwe_add_v", _I, [_P, _P, _P, C.POINTER(_P), C.POINTER(_U64)]),
    ("spf_pool_submit_mul_xn_v", _I, [_P, _P, _SZ, C.POINTER(_P), C.POINTER(_U64)]),
    ("spf_pool_submit_multiply_ggsw_glwe_v", _I, [_P, _P, _P, C.POINTER(_P), C.POINTER(_U64)]),
    ("spf_pool_submit_glev_cmux_v", _I, [_P, _P, _P, _P, C.POINTER(_P), C.POINTER(_U64)]),
    ("spf_pool_submit_scheme_switch_v", _I, [_P, _P, C.POINTER(_P), C.POINTER(_U64)]),
    ("spf_pool_submit_glwe_keyswitch_v", _I, [_P, _U32, _P, C.POINTER(_P), C.POINTER(_U64)]),
    ("spf_pool_submit_glwe_automorphism_v", _I, [_P, _U32, _P, C.POINTER(_P), C.POINTER(_U64)]),
    ("spf_pool_submit_glwe_trace_v", _I, [_P, _P, C.POINTER(_P), C.POINTER(_U64)]),
    ("spf_pool_submit_op_v", _I, [_P, _I, C.POINTER(_P), _SZ, _U64, C.POINTER(_P), C.POINTER(_U64)]),
    ("spf_pool_submit_blind_rotation_v", _I, [_P, _P, C.POINTER(_P), _SZ, _SZ, C.POINTER(_P), C.POINTER(_U64)]),
]


def load_library(path: Optional[str] = None):
    """dlopen the HIP library and declare every prototype.  Raises if it has not been built —
    the product path never falls back to a CPU implementation."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    p = path or lib_path()
    if not os.path.exists(p):
        raise SpfError(-1, f"{p} is missing: build it with spf_amd.build_library() "
                           "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(p)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)  # AttributeError if the header and the library disagree
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _LIB = lib
    return lib


def _u64(a, shape=None) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if shape is not None and a.shape != shape:
        raise ValueError(f"expected shape {shape}, got {a.shape}")
    return a


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _same_rows(what: str, *arrays):
    """the C side copies B * row_size bytes of every operand: a batch mismatch would be an out-of-bounds
    host read (the reference panics in assert_is_valid instead)"""
    rows = {a.shape[0] for a in arrays}
    if len(rows) != 1:
        raise SpfError(-2, f"{what}: operand batches differ in size {[a.shape[0] for a in arrays]}")


def _out(what: str, output, dtype, words: int) -> np.ndarray:
    """caller-allocated output of a pool call: right dtype, C-contiguous, exactly `words` elements"""
    if not isinstance(output, np.ndarray) or output.dtype != np.dtype(dtype) or not output.flags["C_CONTIGUOUS"] \
            or not output.flags["WRITEABLE"] or output.size != words:
        raise SpfError(-2, f"{what}: output must be a writable C-contiguous {np.dtype(dtype).name} array of {words} "
                           f"elements, got {getattr(output, 'dtype', type(output))} x {getattr(output, 'size', '?')}")
    return output


def _in(what: str, a, dtype, words: int) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.size != words:
        raise SpfError(-2, f"{what}: input has {a.size} elements, expected {words}")
    return a


def generate_lut(maps, plaintext_bits: int, params: Params = DEFAULT_128) -> np.ndarray:
    """`generate_lut` (programmable_bootstrapping.rs:129-185) as the trivial GLWE `pbs_univariate` takes.
    `maps`: callables x -> f(x) on [0, 2^plaintext_bits), or already tabulated rows.  Host only, no GPU."""
    lib = load_library()
    p = 1 << plaintext_bits
    table = np.array([[m(x) for x in range(p)] if callable(m) else list(m) for m in maps], dtype=np.uint64).reshape(len(maps), p)
    out = np.empty(params.glwe_words, dtype=np.uint64)
    cp = _CParams(*[getattr(params, n) for n, _ in _CParams._fields_])
    st = lib.spf_generate_lut(C.byref(cp), _ptr(table), len(maps), plaintext_bits, _ptr(out))
    if st != 0:
        raise SpfError(st, (lib.spf_last_error(None) or b"").decode())
    return out


def generate_bivariate_lut(f_or_table, plaintext_bits: int, carry_bits: int, params: Params = DEFAULT_128) -> np.ndarray:
    """`BivariateLookupTable::trivial_from_fn` (entities/bivariate_lookup_table.rs:36-90) = `generate_bivariate_lut`
    (programmable_bootstrapping.rs:413-452) as the trivial GLWE `pbs_bivariate` takes.  `f_or_table`: a callable
    (l, r) -> f(l, r) on [0, 2^plaintext_bits)^2, or its table with table[l][r] = f(l, r) (2^p x 2^p or flat).
    Needs 1 <= plaintext_bits <= carry_bits, 2^(plaintext_bits + carry_bits) <= N and f(l, r) < 2^plaintext_bits.
    Host only, no GPU."""
    lib = load_library()
    # a callable is tabulated only over a plaintext space the C side can accept: otherwise it refuses with its message
    ok = 1 <= plaintext_bits <= carry_bits and (1 << (plaintext_bits + carry_bits)) <= params.polynomial_degree
    p = 1 << plaintext_bits if ok else 1
    if callable(f_or_table):
        table = np.array([f_or_table(l, r) for l in range(p) for r in range(p)] if ok else [0], dtype=np.uint64)
    else:
        table = np.ascontiguousarray(f_or_table, dtype=np.uint64).reshape(-1)
        if ok and table.size != p * p:
            raise SpfError(-2, f"generate_bivariate_lut: the table has {table.size} values, expected 2^(2 * {plaintext_bits})")
    out = np.empty(params.glwe_words, dtype=np.uint64)
    st = lib.spf_generate_bivariate_lut(C.byref(_cparams(params)), _ptr(table), plaintext_bits, carry_bits, _ptr(out))
    if st != 0:
        raise SpfError(st, (lib.spf_last_error(None) or b"").decode())
    return out


def _cparams(params: Params) -> _CParams:
    return _CParams(*[getattr(params, n) for n, _ in _CParams._fields_])


def ciphertext_words(kind: int, params: Params = DEFAULT_128) -> int:
    return int(load_library().spf_ciphertext_words(C.byref(_cparams(params)), int(kind)))


def ciphertext_from_bincode(kind: int, blob: bytes, params: Params = DEFAULT_128) -> np.ndarray:
    """`safe_bincode::deserialize::<L0Lwe | L1Lwe | L1Glwe | L1Glev Ciphertext>` (safe_bincode.rs:16-28,
    encryption.rs:23-110): bytes -> u64 words.  Host only.  Malformed input raises SpfError."""
    lib = load_library()
    n = ciphertext_words(kind, params)
    out = np.empty(max(n, 1), dtype=np.uint64)
    buf = np.frombuffer(bytes(blob) if len(blob) else b"\0", dtype=np.uint8)
    st = lib.spf_ciphertext_from_bincode(C.byref(_cparams(params)), int(kind), _ptr(buf), len(blob), _ptr(out))
    if st != 0:
        raise SpfError(st, (lib.spf_last_error(None) or b"").decode())
    return out[:n]


def ciphertext_to_bincode(kind: int, words, params: Params = DEFAULT_128) -> bytes:
    """`bincode::serialize` of one of the serializable ciphertext newtypes (fixint): u64 count + words, little-endian."""
    lib = load_library()
    n = ciphertext_words(kind, params)
    w = _in("ciphertext", words, np.uint64, max(n, 1)) if n else np.zeros(1, dtype=np.uint64)
    out = np.empty(8 + 8 * n, dtype=np.uint8)
    written = _SZ(0)
    st = lib.spf_ciphertext_to_bincode(C.byref(_cparams(params)), int(kind), _ptr(w), _ptr(out), out.size, C.byref(written))
    if st != 0:
        raise SpfError(st, (lib.spf_last_error(None) or b"").decode())
    return out[:written.value].tobytes()


def live_objects() -> dict:
    """`spf_live_objects`: how many contexts, groups, graphs, pools and values exist in this process (made, not yet freed)"""
    a = (_U64 * 5)()
    st = load_library().spf_live_objects(C.byref(a))
    if st != 0:
        raise SpfError(st, "spf_live_objects failed")
    return dict(zip(("contexts", "groups", "graphs", "pools", "values"), (int(x) for x in a)))


class Engine:
    """One GPU's bootstrap engine (`spf_ctx`)."""

    def __init__(self, params: Params = DEFAULT_128, device: int = 0):
        self._lib = load_library()
        self.params = params
        self.device = device
        cp = _CParams(*[getattr(params, n) for n, _ in _CParams._fields_])
        h = C.c_void_p()
        st = self._lib.spf_create(C.byref(cp), device, C.byref(h))
        if st != 0:
            raise SpfError(st, (self._lib.spf_last_error(None) or b"").decode())
        self._h = h

    # -- plumbing
    def _ck(self, st: int):
        if st != 0:
            raise SpfError(st, (self._lib.spf_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.spf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def version(self) -> str:
        return self._lib.spf_version().decode()

    # -- keys (ComputeKey fields, crypto/keys.rs:306-318)
    def load_bootstrap_key(self, bsk_fft: np.ndarray):
        a = np.ascontiguousarray(bsk_fft, dtype=np.complex128).reshape(-1)
        self._ck(self._lib.spf_load_bootstrap_key(self._h, _ptr(a), a.size))

    def load_keyswitch_key(self, ksk: np.ndarray):
        a = _u64(ksk).reshape(-1)
        self._ck(self._lib.spf_load_keyswitch_key(self._h, _ptr(a), a.size))

    def load_automorphism_key(self, ak_fft: np.ndarray):
        a = np.ascontiguousarray(ak_fft, dtype=np.complex128).reshape(-1)
        self._ck(self._lib.spf_load_automorphism_key(self._h, _ptr(a), a.size))

    def load_scheme_switch_key(self, ssk_fft: np.ndarray):
        a = np.ascontiguousarray(ssk_fft, dtype=np.complex128).reshape(-1)
        self._ck(self._lib.spf_load_scheme_switch_key(self._h, _ptr(a), a.size))

    # -- keys in standard (integer) form (ComputeKeyNonFft fields, crypto/keys.rs:145-159): transformed on the device
    def _std_words(self, what: str, words, want_complex: int) -> np.ndarray:
        if not isinstance(words, np.ndarray) or words.dtype != np.uint64:
            raise SpfError(-2, f"{what}: a standard-form key is a uint64 array, got {getattr(words, 'dtype', type(words))}")
        return _in(what, words, np.uint64, 2 * want_complex).reshape(-1)

    def load_bootstrap_key_std(self, bsk: np.ndarray):
        """`BootstrapKey<u64>` words ([i<n][row][level][poly][N]); `BootstrapKey::fft` happens on the device"""
        a = self._std_words("load_bootstrap_key_std", bsk, self.params.bsk_complex)
        self._ck(self._lib.spf_load_bootstrap_key_std(self._h, _ptr(a), a.size))

    def load_automorphism_key_std(self, ak: np.ndarray):
        a = self._std_words("load_automorphism_key_std", ak, self.params.ak_complex)
        self._ck(self._lib.spf_load_automorphism_key_std(self._h, _ptr(a), a.size))

    def load_scheme_switch_key_std(self, ssk: np.ndarray):
        a = self._std_words("load_scheme_switch_key_std", ssk, self.params.ssk_complex)
        self._ck(self._lib.spf_load_scheme_switch_key_std(self._h, _ptr(a), a.size))

    def load_public_functional_keyswitch_key_std(self, key: np.ndarray, radix_log: int, radix_count: int):
        """`PublicFunctionalKeyswitchKey<u64>` words (from_dimension, radix_count, k+1, N) (sunscreen_tfhe
        entities/public_functional_keyswitch_key.rs); transformed on the device.  The radix belongs to the key."""
        N, k = self.params.polynomial_degree, self.params.glwe_size
        if (not isinstance(key, np.ndarray) or key.dtype != np.uint64 or key.ndim != 4
                or key.shape[1:] != (int(radix_count), k + 1, N)):
            raise SpfError(-2, f"load_public_functional_keyswitch_key_std: the key is a uint64 array of shape "
                               f"(from_dimension, {radix_count}, {k + 1}, {N}), got "
                               f"{getattr(key, 'dtype', type(key))} {getattr(key, 'shape', '')}")
        a = np.ascontiguousarray(key).reshape(-1)
        self._pufks_n = None
        self._ck(self._lib.spf_load_public_functional_keyswitch_key_std(self._h, _ptr(a), a.size, key.shape[0], int(radix_log),
                                                                        int(radix_count)))
        self._pufks_n = int(key.shape[0])

    def load_private_functional_keyswitch_keys_std(self, keys: np.ndarray, radix_log: int, radix_count: int):
        """n_keys x `PrivateFunctionalKeyswitchKey<u64>` words (n_keys, lwe_count, from_dimension + 1, radix_count, k+1, N)
        (sunscreen_tfhe entities/private_functional_keyswitch_key.rs:44-46); integer form, used as it is.  The radix belongs to
        the keys.  (k+1, 1, k*N + 1, ...) is `CircuitBootstrappingKeyswitchKeys<u64>`."""
        N, k = self.params.polynomial_degree, self.params.glwe_size
        if (not isinstance(keys, np.ndarray) or keys.dtype != np.uint64 or keys.ndim != 6
                or keys.shape[3:] != (int(radix_count), k + 1, N)):
            raise SpfError(-2, f"load_private_functional_keyswitch_keys_std: the keys are a uint64 array of shape (n_keys, "
                               f"lwe_count, from_dimension + 1, {radix_count}, {k + 1}, {N}), got "
                               f"{getattr(keys, 'dtype', type(keys))} {getattr(keys, 'shape', '')}")
        a = np.ascontiguousarray(keys).reshape(-1)
        self._pfks_shape = None
        self._ck(self._lib.spf_load_private_functional_keyswitch_keys_std(self._h, _ptr(a), a.size, keys.shape[0], keys.shape[2] - 1,
                                                                          keys.shape[1], int(radix_log), int(radix_count)))
        self._pfks_shape = (int(keys.shape[0]), int(keys.shape[1]), int(keys.shape[2]) - 1)

    def load_compute_key_nonfft_bincode(self, blob: bytes):
        """the bytes `bincode` wrote for a parasol_runtime::ComputeKeyNonFft (keys.rs:145-159), all four keys"""
        buf = np.frombuffer(blob, dtype=np.uint8)
        self._ck(self._lib.spf_load_compute_key_nonfft_bincode(self._h, _ptr(buf), buf.size))

    def poly_fft(self, polys) -> np.ndarray:
        """`PolynomialRef::fft` of every polynomial: uint64 (..., N) -> complex128 (..., N/2)"""
        N = self.params.polynomial_degree
        if not isinstance(polys, np.ndarray) or polys.dtype != np.uint64 or polys.ndim == 0 or polys.shape[-1] != N:
            raise SpfError(-2, f"poly_fft: operand must be a uint64 array of shape (..., {N}), got "
                               f"{getattr(polys, 'dtype', type(polys))} {getattr(polys, 'shape', '')}")
        x = np.ascontiguousarray(polys)
        out = np.empty(x.shape[:-1] + (N // 2,), dtype=np.complex128)
        self._ck(self._lib.spf_poly_fft_batch(self._h, x.size // N, _ptr(x), _ptr(out)))
        return out

    def poly_fft_dev(self, stream, n_polys: int, d_in: int, d_out: int):
        """device pointers; d_out == d_in transforms in place"""
        self._ck(self._lib.spf_poly_fft_dev(self._h, stream, n_polys, d_in, d_out))

    def key_blob(self, which: int):
        """(device pointer, bytes) of the device-resident key; for RCCL broadcast."""
        p, n = C.c_void_p(), C.c_size_t()
        self._ck(self._lib.spf_key_blob(self._h, which, C.byref(p), C.byref(n)))
        return p.value, n.value

    def key_blob_commit(self, which: int):
        self._ck(self._lib.spf_key_blob_commit(self._h, which))

    # -- host-array batch forms
    def keyswitch_lwe_l1_lwe_l0(self, lwe1: np.ndarray) -> np.ndarray:
        x = _u64(lwe1)
        x = x.reshape(-1, self.params.lwe1_words)
        out = np.empty((x.shape[0], self.params.lwe0_words), dtype=np.uint64)
        self._ck(self._lib.spf_keyswitch_lwe_l1_lwe_l0_batch(self._h, x.shape[0], _ptr(x), _ptr(out)))
        return out

    def _lut(self, lut, B):
        lut = _u64(lut)
        if lut.ndim == 1:
            if lut.size != self.params.glwe_words:
                raise ValueError("lut must hold one GLWE")
            return lut, 0
        if lut.shape != (B, self.params.glwe_words):
            raise ValueError("per-ciphertext luts must be B x glwe_words")
        return lut, self.params.glwe_words

    def generalized_pbs(self, lwe0, lut_glwe, log_chi=0, log_v=0, body_rotate=0) -> np.ndarray:
        x = _u64(lwe0).reshape(-1, self.params.lwe0_words)
        lut, stride = self._lut(lut_glwe, x.shape[0])
        out = np.empty((x.shape[0], self.params.glwe_words), dtype=np.uint64)
        self._ck(self._lib.spf_generalized_pbs_batch(self._h, x.shape[0], _ptr(x), _ptr(lut), stride,
                                                     log_chi, log_v, body_rotate, _ptr(out)))
        return out

    def pbs_univariate(self, lwe0, lut_glwe) -> np.ndarray:
        x = _u64(lwe0).reshape(-1, self.params.lwe0_words)
        lut, stride = self._lut(lut_glwe, x.shape[0])
        out = np.empty((x.shape[0], self.params.lwe1_words), dtype=np.uint64)
        self._ck(self._lib.spf_pbs_univariate_batch(self._h, x.shape[0], _ptr(x), _ptr(lut), stride,
                                                    _ptr(out)))
        return out

    def pbs_bivariate(self, left, right, lut_glwe, plaintext_bits: int) -> np.ndarray:
        """`programmable_bootstrap_bivariate` (programmable_bootstrapping.rs:575-621) of each pair (left[i], right[i])"""
        x = _u64(left).reshape(-1, self.params.lwe0_words)
        y = _u64(right).reshape(-1, self.params.lwe0_words)
        _same_rows("pbs_bivariate", x, y)
        lut, stride = self._lut(lut_glwe, x.shape[0])
        out = np.empty((x.shape[0], self.params.lwe1_words), dtype=np.uint64)
        self._ck(self._lib.spf_pbs_bivariate_batch(self._h, x.shape[0], _ptr(x), _ptr(y), _ptr(lut), stride,
                                                   plaintext_bits, _ptr(out)))
        return out

    def circuit_bootstrap_pbs(self, lwe0, out: Optional[np.ndarray] = None) -> np.ndarray:
        """`out`: caller-allocated (B, glwe_words) uint64 array, as the C ABI's caller does — a fresh np.empty is
        untouched memory, and its first-touch page faults land inside the device-to-host copy"""
        x = _u64(lwe0).reshape(-1, self.params.lwe0_words)
        if out is None:
            out = np.empty((x.shape[0], self.params.glwe_words), dtype=np.uint64)
        else:
            _out("circuit_bootstrap_pbs", out, np.uint64, x.shape[0] * self.params.glwe_words)
        self._ck(self._lib.spf_circuit_bootstrap_pbs_batch(self._h, x.shape[0], _ptr(x), _ptr(out)))
        return out

    def circuit_bootstrap(self, lwe0) -> np.ndarray:
        """Evaluation::circuit_bootstrap: L0 LWE -> L1 GGSW-FFT (B x cbs_ggsw_complex)."""
        x = _u64(lwe0).reshape(-1, self.params.lwe0_words)
        out = np.empty((x.shape[0], self.params.cbs_ggsw_complex), dtype=np.complex128)
        self._ck(self._lib.spf_circuit_bootstrap_batch(self._h, x.shape[0], _ptr(x), _ptr(out)))
        return out

    def mod_switch_trace_and_rotate(self, glwe) -> np.ndarray:
        x = _u64(glwe).reshape(-1, self.params.glwe_words)
        out = np.empty((x.shape[0], self.params.cbs_radix_count, self.params.glwe_words), dtype=np.uint64)
        self._ck(self._lib.spf_mod_switch_trace_and_rotate_batch(self._h, x.shape[0], _ptr(x), _ptr(out)))
        return out

    def scheme_switch(self, glev) -> np.ndarray:
        x = _u64(glev).reshape(-1, self.params.cbs_radix_count * self.params.glwe_words)
        out = np.empty((x.shape[0], self.params.cbs_ggsw_complex), dtype=np.complex128)
        self._ck(self._lib.spf_scheme_switch_batch(self._h, x.shape[0], _ptr(x), _ptr(out)))
        return out

    def sample_extract_l1(self, glwe, idx: int) -> np.ndarray:
        x = _u64(glwe).reshape(-1, self.params.glwe_words)
        out = np.empty((x.shape[0], self.params.lwe1_words), dtype=np.uint64)
        self._ck(self._lib.spf_sample_extract_l1_batch(self._h, x.shape[0], _ptr(x), idx, _ptr(out)))
        return out

    def glwe_not(self, glwe) -> np.ndarray:
        x = _u64(glwe).reshape(-1, self.params.glwe_words)
        out = np.empty_like(x)
        self._ck(self._lib.spf_glwe_not_batch(self._h, x.shape[0], _ptr(x), _ptr(out)))
        return out

    def glwe_xor(self, a, b) -> np.ndarray:
        a = _u64(a).reshape(-1, self.params.glwe_words)
        b = _u64(b).reshape(-1, self.params.glwe_words)
        if a.shape != b.shape:
            raise SpfError(-2, "glwe_xor: operand batches differ in size")
        out = np.empty_like(a)
        self._ck(self._lib.spf_glwe_xor_batch(self._h, a.shape[0], _ptr(a), _ptr(b), _ptr(out)))
        return out

    def glwe_mul_xn(self, glwe, n: int) -> np.ndarray:
        x = _u64(glwe).reshape(-1, self.params.glwe_words)
        out = np.empty_like(x)
        self._ck(self._lib.spf_glwe_mul_xn_batch(self._h, x.shape[0], _ptr(x), n, _ptr(out)))
        return out

    def cmux(self, sel_ggsw_fft, a, b) -> np.ndarray:
        g = np.ascontiguousarray(sel_ggsw_fft, dtype=np.complex128).reshape(-1, self.params.cbs_ggsw_complex)
        a = _u64(a).reshape(-1, self.params.glwe_words)
        b = _u64(b).reshape(-1, self.params.glwe_words)
        _same_rows("cmux", g, a, b)
        out = np.empty_like(a)
        self._ck(self._lib.spf_cmux_batch(self._h, a.shape[0], _ptr(g), _ptr(a), _ptr(b), _ptr(out)))
        return out

    def glev_cmux(self, sel_ggsw_fft, a, b) -> np.ndarray:
        n = self.params.cbs_radix_count * self.params.glwe_words
        g = np.ascontiguousarray(sel_ggsw_fft, dtype=np.complex128).reshape(-1, self.params.cbs_ggsw_complex)
        a = _u64(a).reshape(-1, n)
        b = _u64(b).reshape(-1, n)
        _same_rows("glev_cmux", g, a, b)
        out = np.empty_like(a)
        self._ck(self._lib.spf_glev_cmux_batch(self._h, a.shape[0], _ptr(g), _ptr(a), _ptr(b), _ptr(out)))
        return out

    def multiply_glwe_ggsw(self, glwe, ggsw_fft) -> np.ndarray:
        g = np.ascontiguousarray(ggsw_fft, dtype=np.complex128).reshape(-1, self.params.cbs_ggsw_complex)
        x = _u64(glwe).reshape(-1, self.params.glwe_words)
        _same_rows("multiply_glwe_ggsw", g, x)
        out = np.empty_like(x)
        self._ck(self._lib.spf_multiply_glwe_ggsw_batch(self._h, x.shape[0], _ptr(x), _ptr(g), _ptr(out)))
        return out

    def keyswitch_circuit_bootstrap(self, lwe1) -> np.ndarray:
        """KeyswitchL1toL0 -> CircuitBootstrap (L1 LWE in, L1 GGSW-FFT out); the L0 LWE stays on the device"""
        x = _u64(lwe1).reshape(-1, self.params.lwe1_words)
        out = np.empty((x.shape[0], self.params.cbs_ggsw_complex), dtype=np.complex128)
        self._ck(self._lib.spf_keyswitch_circuit_bootstrap_batch(self._h, x.shape[0], _ptr(x), _ptr(out)))
        return out

    # -- packed integers (int-major: bit i of packed ciphertext b is [b, i]; spf_amd.packed has the plaintext side)
    def glwe_pack(self, bits) -> np.ndarray:
        """`DynamicGenericIntGraphNodes::pack` (fluent/dynamic_generic_int_graph_nodes.rs:139-200): (B, n, glwe_words)
        GLWEs of the bits -> (B, glwe_words), the sum of bit i's GLWE times X^i"""
        x = _u64(bits)
        if x.ndim != 3 or x.shape[2] != self.params.glwe_words:
            raise SpfError(-2, f"glwe_pack: bits must have shape (B, n_bits, {self.params.glwe_words}), got {x.shape}")
        out = np.empty((x.shape[0], self.params.glwe_words), dtype=np.uint64)
        self._ck(self._lib.spf_glwe_pack_batch(self._h, x.shape[0], x.shape[1], _ptr(x), _ptr(out)))
        return out

    def glwe_unpack_l1(self, packed, n_bits: int) -> np.ndarray:
        """`PackedDynamicGenericIntGraphNode::unpack` (fluent/packed_dynamic_generic_int_graph_node.rs:24-39):
        (B, glwe_words) -> (B, n_bits, lwe1_words), [b, i] = sample_extract(packed[b], i)"""
        x = _u64(packed).reshape(-1, self.params.glwe_words)
        out = np.empty((x.shape[0], n_bits, self.params.lwe1_words), dtype=np.uint64)
        self._ck(self._lib.spf_glwe_unpack_l1_batch(self._h, x.shape[0], n_bits, _ptr(x), _ptr(out)))
        return out

    def unpack_circuit_bootstrap(self, packed, n_bits: int) -> np.ndarray:
        """unpack, then KeyswitchL1toL0 -> CircuitBootstrap of every bit: (B, glwe_words) -> (B, n_bits, cbs_ggsw_complex),
        the GGSWs a mux circuit reads; the LWEs stay on the device"""
        x = _u64(packed).reshape(-1, self.params.glwe_words)
        out = np.empty((x.shape[0], n_bits, self.params.cbs_ggsw_complex), dtype=np.complex128)
        self._ck(self._lib.spf_unpack_circuit_bootstrap_batch(self._h, x.shape[0], n_bits, _ptr(x), _ptr(out)))
        return out

    def blind_rotation(self, shift_ggsw_fft, glwe, log_stride: int = 0) -> np.ndarray:
        """`blind_rotation` (sunscreen_tfhe ops/bootstrapping/blind_rotation.rs:202-223): glwe[b] * X^-(s_b << log_stride), the
        shift s_b given as the GGSWs of its bits, least significant first (what unpack_circuit_bootstrap returns):
        (B, n_bits, cbs_ggsw_complex) and (B, glwe_words) -> (B, glwe_words); spf_amd.packed.trivial_table_glwe makes a table
        whose entry s_b this brings to coefficient 0"""
        g = np.ascontiguousarray(shift_ggsw_fft, dtype=np.complex128)
        if g.ndim != 3 or g.shape[2] != self.params.cbs_ggsw_complex:
            raise SpfError(-2, f"blind_rotation: shift must have shape (B, n_bits, {self.params.cbs_ggsw_complex}), got {g.shape}")
        x = _u64(glwe).reshape(-1, self.params.glwe_words)
        _same_rows("blind_rotation", g, x)
        out = np.empty_like(x)
        self._ck(self._lib.spf_blind_rotation_batch(self._h, x.shape[0], g.shape[1], int(log_stride), _ptr(g), _ptr(x), _ptr(out)))
        return out

    def public_functional_keyswitch(self, lwes) -> np.ndarray:
        """`public_functional_keyswitch` (sunscreen_tfhe ops/keyswitch/public_functional_keyswitch.rs:74-148), message j to
        coefficient j: (B, lwe_count, from_dimension + 1) LWEs -> (B, glwe_words), one GLWE per row of lwe_count <= N LWEs"""
        n = getattr(self, "_pufks_n", None)
        if n is None:
            raise SpfError(3, "public functional keyswitch key not loaded")
        x = _u64(lwes)
        if x.ndim != 3 or x.shape[2] != n + 1:
            raise SpfError(-2, f"public_functional_keyswitch: operand must have shape (B, lwe_count, {n + 1}), got {x.shape}")
        out = np.empty((x.shape[0], self.params.glwe_words), dtype=np.uint64)
        self._ck(self._lib.spf_public_functional_keyswitch_batch(self._h, x.shape[0], x.shape[1], _ptr(x), _ptr(out)))
        return out

    def _pfks(self):
        shape = getattr(self, "_pfks_shape", None)
        if shape is None:
            raise SpfError(3, "private functional keyswitch keys not loaded")
        return shape

    def private_functional_keyswitch(self, lwes, key_index: int = 0) -> np.ndarray:
        """`private_functional_keyswitch` (sunscreen_tfhe ops/keyswitch/private_functional_keyswitch.rs:107-142) under key
        `key_index`: (B, lwe_count, from_dimension + 1) LWEs -> (B, glwe_words)"""
        _, p, n = self._pfks()
        x = _u64(lwes)
        if x.ndim != 3 or x.shape[1:] != (p, n + 1):
            raise SpfError(-2, f"private_functional_keyswitch: operand must have shape (B, {p}, {n + 1}), got {x.shape}")
        out = np.empty((x.shape[0], self.params.glwe_words), dtype=np.uint64)
        self._ck(self._lib.spf_private_functional_keyswitch_batch(self._h, int(key_index), x.shape[0], _ptr(x), _ptr(out)))
        return out

    def apply_pfks_on_ggsw_components(self, lwes) -> np.ndarray:
        """`apply_pfks_on_ggsw_components` (ops/bootstrapping/circuit_bootstrapping.rs:485-514): (B, l_cbs, k*N + 1) LWEs ->
        (B, k+1, l_cbs, k+1, N) integer-form GGSWs"""
        _, _, n = self._pfks()
        N, k, L = self.params.polynomial_degree, self.params.glwe_size, self.params.cbs_radix_count
        x = _u64(lwes)
        if x.ndim != 3 or x.shape[1:] != (L, n + 1):
            raise SpfError(-2, f"apply_pfks_on_ggsw_components: operand must have shape (B, {L}, {n + 1}), got {x.shape}")
        out = np.empty((x.shape[0], k + 1, L, k + 1, N), dtype=np.uint64)
        self._ck(self._lib.spf_apply_pfks_on_ggsw_components_batch(self._h, x.shape[0], _ptr(x), _ptr(out)))
        return out

    def circuit_bootstrap_via_pfks(self, lwe0) -> np.ndarray:
        """`circuit_bootstrap_via_pfks` (ops/bootstrapping/circuit_bootstrapping.rs:162-219): (B, lwe0_words) -> GGSW spectra in
        the layout `cmux` consumes, as `circuit_bootstrap` returns them"""
        self._pfks()
        x = _u64(lwe0).reshape(-1, self.params.lwe0_words)
        out = np.empty((x.shape[0], self.params.cbs_ggsw_complex), dtype=np.complex128)
        self._ck(self._lib.spf_circuit_bootstrap_via_pfks_batch(self._h, x.shape[0], _ptr(x), _ptr(out)))
        return out

    def load_lwe_linear_weights(self, slot: int, weights, bias=None):
        """weights of a plaintext linear map (`scalar_mul_ciphertext_mad` + `add_lwe_inplace`, sunscreen_tfhe
        ops/ciphertext/lwe_ciphertext_ops.rs:48-66, :4-18) into slot `slot` < LWE_LINEAR_SLOTS: an (M, K) int64 matrix and an
        optional bias of M uint64 words.  Replaces what the slot held; synchronous."""
        w = np.asarray(weights)
        if w.ndim != 2 or w.dtype.kind not in "iu" or (w.dtype.kind == "u" and w.size and int(w.max()) > 2**63 - 1):
            raise SpfError(-2, f"load_lwe_linear_weights: the weights are a 2-D array of int64 values, got {w.dtype} {w.shape}")
        w = np.ascontiguousarray(w, dtype=np.int64)
        b = None
        if bias is not None:
            b = _u64(bias)
            if b.shape != (w.shape[0],):
                raise SpfError(-2, f"load_lwe_linear_weights: the bias has shape {b.shape}, expected ({w.shape[0]},)")
        shapes = self.__dict__.setdefault("_lin_shapes", {})
        shapes.pop(int(slot), None)
        self._ck(self._lib.spf_load_lwe_linear_weights(self._h, int(slot), w.shape[0], w.shape[1], _ptr(w), _ptr(b) if b is not None else None))
        shapes[int(slot)] = (int(w.shape[0]), int(w.shape[1]))

    def lwe_linear_slot_shape(self, slot: int):
        """`spf_lwe_linear_slot_shape`: (M, K, has_bias) of the weights in `slot`; an empty slot is SPF_ERR_NO_KEY"""
        M, K, has_bias = _SZ(), _SZ(), C.c_int()
        self._ck(self._lib.spf_lwe_linear_slot_shape(self._h, int(slot) & 0xFFFFFFFF, C.byref(M), C.byref(K), C.byref(has_bias)))
        return int(M.value), int(K.value), bool(has_bias.value)

    def _lin(self, slot: int, kind: int):
        """(M, K, W) of a loaded slot for ciphertexts of `kind`; whatever the library refuses is refused by the library"""
        shape = self.__dict__.get("_lin_shapes", {}).get(int(slot)) if 0 <= int(slot) < 2**32 else None
        if int(kind) not in (VAL_LWE0, VAL_LWE1):   # (the slot first, then the kind: the order of the batch call's own checks)
            one = np.zeros(1, dtype=np.uint64)
            two = np.zeros(1, dtype=np.uint64)
            self._ck(self._lib.spf_lwe_linear_batch(self._h, int(slot) & 0xFFFFFFFF, int(kind), 0, _ptr(one), _ptr(two)))
            raise SpfError(1, f"lwe_linear: kind {kind} is not an LWE kind")
        if shape is None:   # not loaded through this handle: the library knows
            shape = self.lwe_linear_slot_shape(slot)[:2]
        return shape + (self.params.lwe0_words if int(kind) == VAL_LWE0 else self.params.lwe1_words,)

    def lwe_linear(self, slot: int, lwes, kind: int = 0) -> np.ndarray:
        """out[b][m] = sum_k w[m][k] * lwes[b][k] (+ bias[m] on the body), every word mod 2^64: (B, K, W) LWEs of one kind
        (VAL_LWE0: W = n+1, VAL_LWE1: W = k*N+1) -> (B, M, W), under the weights of slot `slot`"""
        M, K, W = self._lin(slot, kind)
        x = _u64(lwes)
        if x.ndim != 3 or x.shape[1:] != (K, W):
            raise SpfError(-2, f"lwe_linear: operand must have shape (B, {K}, {W}), got {x.shape}")
        out = np.empty((x.shape[0], M, W), dtype=np.uint64)
        self._ck(self._lib.spf_lwe_linear_batch(self._h, int(slot), int(kind), x.shape[0], _ptr(x), _ptr(out)))
        return out

    def load_glwe_poly_weights(self, slot: int, w, bias=None, shape=None):
        """weights of a plaintext polynomial linear map over GLWE ciphertexts (`glwe_polynomial_mad`, `glwe_scalar_mad`,
        `sub_glwe_ciphertexts`, `glwe_negate_inplace`, `glwe_rotate`; sunscreen_tfhe ops/ciphertext/glwe_ciphertext_ops.rs:164-183,
        :189-202, :121-141, :147-156, :285-305) into slot `slot` < GLWE_POLY_SLOTS.  `w` is a dense (M, K, N) array of int64
        coefficients, of which the non-zeros are kept, or the CSR triple (offsets, exponents, coefficients) over the M * K
        polynomials with `shape` = (M, K).  `bias`: M plaintext polynomials, (M, N) uint64 words, added to the body.
        Replaces what the slot held; synchronous."""
        N = self.params.polynomial_degree
        if isinstance(w, tuple):
            if len(w) != 3 or shape is None or len(shape) != 2:
                raise SpfError(-2, "load_glwe_poly_weights: the sparse form is (offsets, exponents, coefficients) with shape=(M, K)")
            M, K = int(shape[0]), int(shape[1])
            off, exp = (np.asarray(a) for a in w[:2])
            coef = np.asarray(w[2])
            for name, a in (("offsets", off), ("exponents", exp)):
                if a.ndim != 1 or (a.size and (a.dtype.kind not in "iu" or int(a.min()) < 0 or int(a.max()) >= 2**32)):
                    raise SpfError(-2, f"load_glwe_poly_weights: the {name} are a 1-D array of uint32 values")
            if coef.ndim != 1 or (coef.size and coef.dtype.kind not in "iu") or (coef.dtype.kind == "u" and coef.size and int(coef.max()) > 2**63 - 1):
                raise SpfError(-2, "load_glwe_poly_weights: the coefficients are a 1-D array of int64 values")
            if M < 0 or K < 0 or off.size != M * K + 1 or exp.size != coef.size or (off.size and int(off[-1]) > exp.size):
                raise SpfError(-2, f"load_glwe_poly_weights: {off.size} offsets, {exp.size} exponents and {coef.size} coefficients "
                                   f"do not describe {M} x {K} polynomials")
            off, exp = np.ascontiguousarray(off, dtype=np.uint32), np.ascontiguousarray(exp, dtype=np.uint32)
            coef = np.ascontiguousarray(coef, dtype=np.int64)
        else:
            d = np.asarray(w)
            if d.ndim != 3 or d.shape[2] != N or d.dtype.kind not in "iu" or (d.dtype.kind == "u" and d.size and int(d.max()) > 2**63 - 1):
                raise SpfError(-2, f"load_glwe_poly_weights: the dense form is an (M, K, {N}) array of int64 values, got {d.dtype} {d.shape}")
            d = np.ascontiguousarray(d, dtype=np.int64)
            M, K = d.shape[:2]
            nz = d != 0
            off = np.concatenate([[0], np.cumsum(nz.reshape(M * K, N).sum(axis=1))]).astype(np.uint32)
            exp = np.nonzero(nz)[2].astype(np.uint32)
            coef = np.ascontiguousarray(d[nz])
        b = None
        if bias is not None:
            b = _u64(bias)
            if b.shape != (M, N):
                raise SpfError(-2, f"load_glwe_poly_weights: the bias has shape {b.shape}, expected ({M}, {N})")
        keep = np.zeros(1, dtype=np.uint64)   # (an empty array has no address worth passing)
        self._ck(self._lib.spf_load_glwe_poly_weights(self._h, int(slot) & 0xFFFFFFFF, M, K, _ptr(off), _ptr(exp if exp.size else keep),
                                                      _ptr(coef if coef.size else keep), _ptr(b) if b is not None else None))

    def glwe_poly_slot_shape(self, slot: int):
        """`spf_glwe_poly_slot_shape`: (M, K, terms, has_bias) of the weights in `slot`; an empty slot is SPF_ERR_NO_KEY"""
        M, K, T, has_bias = _SZ(), _SZ(), _SZ(), C.c_int()
        self._ck(self._lib.spf_glwe_poly_slot_shape(self._h, int(slot) & 0xFFFFFFFF, C.byref(M), C.byref(K), C.byref(T), C.byref(has_bias)))
        return int(M.value), int(K.value), int(T.value), bool(has_bias.value)

    def glwe_poly_linear(self, slot: int, glwes) -> np.ndarray:
        """out[b][m] = sum_k w[m][k] * glwes[b][k] (+ bias[m] on the body) in Z_2^64[X]/(X^N + 1), word for word: (B, K, k+1, N)
        GLWEs -> (B, M, k+1, N), under the polynomial weights of slot `slot`"""
        M, K = self.glwe_poly_slot_shape(slot)[:2]
        k1, N = self.params.glwe_size + 1, self.params.polynomial_degree
        x = _u64(glwes)
        if x.ndim == 3 and x.shape[1:] == (K, k1 * N):
            x = x.reshape(-1, K, k1, N)
        if x.ndim != 4 or x.shape[1:] != (K, k1, N):
            raise SpfError(-2, f"glwe_poly_linear: operand must have shape (B, {K}, {k1}, {N}), got {x.shape}")
        out = np.empty((x.shape[0], M, k1, N), dtype=np.uint64)
        self._ck(self._lib.spf_glwe_poly_linear_batch(self._h, int(slot), x.shape[0], _ptr(x), _ptr(out)))
        return out

    # GLWE keyswitch, one automorphism round, trace (`keyswitch_glwe_to_glwe`, sunscreen_tfhe ops/fft_ops.rs:457-495; ops/automorphisms/
    # mod.rs:53-85)
    def load_glwe_keyswitch_key_std(self, slot: int, key: np.ndarray, radix_log: int, radix_count: int):
        """`GlweKeyswitchKey<u64>` words (k, radix_count, k+1, N) into slot `slot` < GLWE_KSK_SLOTS; transformed on the device.
        The radix belongs to the key.  Replaces what the slot held; synchronous."""
        N, k = self.params.polynomial_degree, self.params.glwe_size
        if (not isinstance(key, np.ndarray) or key.dtype != np.uint64 or key.ndim != 4
                or key.shape != (k, int(radix_count), k + 1, N)):
            raise SpfError(-2, f"load_glwe_keyswitch_key_std: the key is a uint64 array of shape ({k}, {int(radix_count)}, {k + 1}, {N}), "
                               f"got {getattr(key, 'dtype', type(key))} {getattr(key, 'shape', '')}")
        a = np.ascontiguousarray(key)
        self._ck(self._lib.spf_load_glwe_keyswitch_key_std(self._h, int(slot) & 0xFFFFFFFF, _ptr(a), a.size, int(radix_log), int(radix_count)))

    def glwe_keyswitch_slot_shape(self, slot: int):
        """`spf_glwe_keyswitch_slot_shape`: (radix_log, radix_count) of the key in `slot`; an empty slot is SPF_ERR_NO_KEY"""
        lg, cnt = _U32(), _U32()
        self._ck(self._lib.spf_glwe_keyswitch_slot_shape(self._h, int(slot) & 0xFFFFFFFF, C.byref(lg), C.byref(cnt)))
        return int(lg.value), int(cnt.value)

    def _glwes(self, name: str, glwes) -> np.ndarray:
        k1, N = self.params.glwe_size + 1, self.params.polynomial_degree
        x = _u64(glwes)
        if x.ndim == 2 and x.shape[1] == k1 * N:
            x = x.reshape(-1, k1, N)
        if x.ndim != 3 or x.shape[1:] != (k1, N):
            raise SpfError(-2, f"{name}: operand must have shape (B, {k1}, {N}), got {x.shape}")
        return x

    def glwe_keyswitch(self, slot: int, glwes) -> np.ndarray:
        """`keyswitch_glwe_to_glwe` of (B, k+1, N) GLWEs under the key of slot `slot`, word for word"""
        x = self._glwes("glwe_keyswitch", glwes)
        out = np.empty_like(x)
        self._ck(self._lib.spf_glwe_keyswitch_batch(self._h, int(slot) & 0xFFFFFFFF, x.shape[0], _ptr(x), _ptr(out)))
        return out

    def glwe_automorphism(self, round: int, glwes) -> np.ndarray:
        """round `round` in 1 .. log2 N of the trace's loop: keyswitch(x(X^t), ak[round - 1]), t = N / 2^(round - 1) + 1"""
        x = self._glwes("glwe_automorphism", glwes)
        out = np.empty_like(x)
        self._ck(self._lib.spf_glwe_automorphism_batch(self._h, int(round) & 0xFFFFFFFF, x.shape[0], _ptr(x), _ptr(out)))
        return out

    # ---- the parameter per item (spf_*_each_batch): ONE launch over B items under B parameters, row i the result of item i under
    # params[i].  `out`: a caller's array to write into (the tests look at the rows around it), else a fresh one.
    def _each(self, name: str, fn, glwes, params, out_words: int, out):
        x = self._glwes(name, glwes)
        try:
            p = np.array([int(v) for v in (params.reshape(-1) if isinstance(params, np.ndarray) else params)], dtype=np.uint64).reshape(-1)
        except (OverflowError, TypeError, ValueError):
            raise SpfError(-2, f"{name}: the parameters must be non-negative integers below 2^64")
        if p.shape[0] != x.shape[0]:
            raise SpfError(-2, f"{name}: {x.shape[0]} items but {p.shape[0]} parameters")
        if out is None:
            out = np.empty((x.shape[0], out_words), dtype=np.uint64)
        else:
            _out(name, out, np.uint64, x.shape[0] * out_words)
        self._ck(fn(self._h, x.shape[0], _ptr(x), _ptr(p), _ptr(out)))
        return out

    def sample_extract_l1_each(self, glwes, idx, out: Optional[np.ndarray] = None) -> np.ndarray:
        """`sample_extract(glwes[i], idx[i])`: replaces one sample_extract_l1 call per distinct index"""
        return self._each("sample_extract_l1_each", self._lib.spf_sample_extract_l1_each_batch, glwes, idx, self.params.lwe1_words, out)

    def glwe_mul_xn_each(self, glwes, amounts, out: Optional[np.ndarray] = None) -> np.ndarray:
        """`glwes[i] * X^amounts[i]`, amounts mod 2N: replaces one glwe_mul_xn call per distinct amount"""
        return self._each("glwe_mul_xn_each", self._lib.spf_glwe_mul_xn_each_batch, glwes, amounts, self.params.glwe_words, out)

    def glwe_keyswitch_each(self, slots, glwes, out: Optional[np.ndarray] = None) -> np.ndarray:
        """item i under the key of slot slots[i]: replaces one glwe_keyswitch call per distinct slot"""
        return self._each("glwe_keyswitch_each", self._lib.spf_glwe_keyswitch_each_batch, glwes, slots, self.params.glwe_words, out)

    def glwe_automorphism_each(self, rounds, glwes, out: Optional[np.ndarray] = None) -> np.ndarray:
        """item i through round rounds[i] of the trace's loop: replaces one glwe_automorphism call per distinct round"""
        return self._each("glwe_automorphism_each", self._lib.spf_glwe_automorphism_each_batch, glwes, rounds, self.params.glwe_words, out)

    def glwe_trace(self, glwes) -> np.ndarray:
        """`trace` (ops/automorphisms/mod.rs:53-85) of (B, k+1, N) GLWEs under the context's automorphism key"""
        x = self._glwes("glwe_trace", glwes)
        out = np.empty_like(x)
        self._ck(self._lib.spf_glwe_trace_batch(self._h, x.shape[0], _ptr(x), _ptr(out)))
        return out

    def lwe_ring_pack(self, leaves, p: int, leaf_kind: int = VAL_LWE1, out: Optional[np.ndarray] = None) -> np.ndarray:
        """ring packing (`spf_lwe_ring_pack_batch`): (B, p, leaf words) LWE1 or GLWE1 leaves into (B, glwe_words) GLWEs under the
        automorphism key; leaf j's message lands at coefficient j * N / p (the strided layout: spf_amd.packed.strided_positions)"""
        p = int(p)
        words = self.params.lwe1_words if int(leaf_kind) == VAL_LWE1 else self.params.glwe_words
        x = _u64(leaves).reshape(-1)
        if p < 1 or x.size % (p * words):
            raise SpfError(-2, f"lwe_ring_pack: {x.size} words are no whole number of outputs of p = {p} leaves of {words} words")
        B = x.size // (p * words)
        if out is None:
            out = np.empty((B, self.params.glwe_words), dtype=np.uint64)
        else:
            _out("lwe_ring_pack", out, np.uint64, B * self.params.glwe_words)
        self._ck(self._lib.spf_lwe_ring_pack_batch(self._h, int(leaf_kind), p, B, _ptr(x), _ptr(out)))
        return out

    def lwe_ring_pack_scratch_words(self, p: int, B: int) -> int:
        w = C.c_size_t()
        self._ck(self._lib.spf_lwe_ring_pack_scratch_words(self._h, int(p), int(B), C.byref(w)))
        return w.value

    def gate_bootstrap(self, lwe1, out: Optional[np.ndarray] = None) -> np.ndarray:
        x = _u64(lwe1).reshape(-1, self.params.lwe1_words)
        if out is None:
            out = np.empty((x.shape[0], self.params.glwe_words), dtype=np.uint64)
        else:
            _out("gate_bootstrap", out, np.uint64, x.shape[0] * self.params.glwe_words)
        self._ck(self._lib.spf_gate_bootstrap_batch(self._h, x.shape[0], _ptr(x), _ptr(out)))
        return out

    # -- device-pointer forms (ints are raw device addresses; stream is a hipStream_t handle)
    def keyswitch_dev(self, stream: int, B: int, d_in: int, d_out: int):
        self._ck(self._lib.spf_keyswitch_lwe_l1_lwe_l0_dev(self._h, stream, B, d_in, d_out))

    def generalized_pbs_dev(self, stream, B, d_lwe, d_lut, lut_stride, log_chi, log_v, body_rotate, d_out):
        self._ck(self._lib.spf_generalized_pbs_dev(self._h, stream, B, d_lwe, d_lut, lut_stride,
                                                   log_chi, log_v, body_rotate, d_out))

    def pbs_univariate_dev(self, stream, B, d_lwe, d_lut, lut_stride, d_out):
        self._ck(self._lib.spf_pbs_univariate_dev(self._h, stream, B, d_lwe, d_lut, lut_stride, d_out))

    def pbs_bivariate_dev(self, stream, B, d_left, d_right, d_lut, lut_stride, plaintext_bits, d_out):
        self._ck(self._lib.spf_pbs_bivariate_dev(self._h, stream, B, d_left, d_right, d_lut, lut_stride, plaintext_bits,
                                                 d_out))

    def circuit_bootstrap_pbs_dev(self, stream: int, B: int, d_lwe: int, d_out: int):
        self._ck(self._lib.spf_circuit_bootstrap_pbs_dev(self._h, stream, B, d_lwe, d_out))

    def circuit_bootstrap_dev(self, stream, B, d_lwe, d_ggsw_out):
        self._ck(self._lib.spf_circuit_bootstrap_dev(self._h, stream, B, d_lwe, d_ggsw_out))

    def mod_switch_trace_and_rotate_dev(self, stream, B, d_glwe, d_glev_out):
        self._ck(self._lib.spf_mod_switch_trace_and_rotate_dev(self._h, stream, B, d_glwe, d_glev_out))

    def scheme_switch_dev(self, stream, B, d_glev, d_ggsw_out):
        self._ck(self._lib.spf_scheme_switch_dev(self._h, stream, B, d_glev, d_ggsw_out))

    def cmux_dev(self, stream, B, d_sel_ggsw_fft, d_a, d_b, d_out):
        self._ck(self._lib.spf_cmux_dev(self._h, stream, B, d_sel_ggsw_fft, d_a, d_b, d_out))

    def cmux_scattered_dev(self, stream, units, d_ptrs):
        """`units` CMUXes over scattered operands: d_ptrs = device array of 4 pointers per unit {selector, a (0 = zero), b, out}"""
        self._ck(self._lib.spf_cmux_scattered_dev(self._h, stream, units, d_ptrs))

    def glwe_not_dev(self, stream, B, d_in, d_out):
        self._ck(self._lib.spf_glwe_not_dev(self._h, stream, B, d_in, d_out))

    def glwe_xor_dev(self, stream, B, d_a, d_b, d_out):
        self._ck(self._lib.spf_glwe_xor_dev(self._h, stream, B, d_a, d_b, d_out))

    def glwe_mul_xn_dev(self, stream, B, d_in, n, d_out):
        self._ck(self._lib.spf_glwe_mul_xn_dev(self._h, stream, B, d_in, n, d_out))

    def sample_extract_l1_dev(self, stream, B, d_glwe, idx, d_out):
        self._ck(self._lib.spf_sample_extract_l1_dev(self._h, stream, B, d_glwe, idx, d_out))

    def glwe_pack_dev(self, stream, B, n_bits, d_bits, d_out):
        self._ck(self._lib.spf_glwe_pack_dev(self._h, stream, B, n_bits, d_bits, d_out))

    def glwe_unpack_l1_dev(self, stream, B, n_bits, d_packed, d_out):
        self._ck(self._lib.spf_glwe_unpack_l1_dev(self._h, stream, B, n_bits, d_packed, d_out))

    def unpack_circuit_bootstrap_dev(self, stream, B, n_bits, d_packed, d_ggsw_out):
        self._ck(self._lib.spf_unpack_circuit_bootstrap_dev(self._h, stream, B, n_bits, d_packed, d_ggsw_out))

    def blind_rotation_dev(self, stream, B, n_bits, log_stride, d_shift, d_in, d_out):
        self._ck(self._lib.spf_blind_rotation_dev(self._h, stream, B, n_bits, log_stride, d_shift, d_in, d_out))

    def public_functional_keyswitch_enqueue(self, stream, B, lwe_count, d_lwe_in, d_glwe_out):
        self._ck(self._lib.spf_public_functional_keyswitch_enqueue(self._h, stream, B, lwe_count, d_lwe_in, d_glwe_out))

    def private_functional_keyswitch_enqueue(self, stream, key_index, B, d_lwe_in, d_glwe_out):
        self._ck(self._lib.spf_private_functional_keyswitch_enqueue(self._h, stream, key_index, B, d_lwe_in, d_glwe_out))

    def apply_pfks_on_ggsw_components_enqueue(self, stream, B, d_lwe_in, d_ggsw_out):
        self._ck(self._lib.spf_apply_pfks_on_ggsw_components_enqueue(self._h, stream, B, d_lwe_in, d_ggsw_out))

    def circuit_bootstrap_via_pfks_enqueue(self, stream, B, d_lwe0_in, d_ggsw_fft_out):
        self._ck(self._lib.spf_circuit_bootstrap_via_pfks_enqueue(self._h, stream, B, d_lwe0_in, d_ggsw_fft_out))

    # -- device buffers (for chaining the _dev forms without a HIP binding of one's own)
    def device_alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self._ck(self._lib.spf_device_alloc(self._h, int(nbytes), C.byref(p)))
        return p.value or 0

    def device_free(self, ptr: int):
        self._ck(self._lib.spf_device_free(self._h, ptr))

    def device_upload(self, ptr: int, host: np.ndarray):
        host = np.ascontiguousarray(host)
        self._ck(self._lib.spf_device_upload(self._h, ptr, _ptr(host), host.nbytes))

    def device_download(self, stream, host: np.ndarray, ptr: int):
        """waits for `stream` (None = the default stream), then copies host.nbytes bytes from `ptr`"""
        assert host.flags.c_contiguous
        self._ck(self._lib.spf_device_download(self._h, stream, _ptr(host), ptr, host.nbytes))

    # -- measurement
    def set_timing(self, enabled: bool):
        self._ck(self._lib.spf_set_timing(self._h, 1 if enabled else 0))

    def load_compute_key_bincode(self, blob: bytes):
        """the bytes `bincode` wrote for a parasol_runtime::ComputeKey (safe_bincode.rs:16-28), all four keys"""
        buf = np.frombuffer(blob, dtype=np.uint8)
        self._ck(self._lib.spf_load_compute_key_bincode(self._h, _ptr(buf), buf.size))

    def l1ggsw_constant(self, bit: int) -> np.ndarray:
        """Evaluation::l1ggsw_zero / l1ggsw_one: circuit bootstrap of the trivial L0 LWE of `bit` (cached per key set)"""
        out = np.empty(self.params.cbs_ggsw_complex, dtype=np.complex128)
        self._ck(self._lib.spf_l1ggsw_constant(self._h, int(bit), _ptr(out)))
        return out

    def last_blind_rotate_kernel(self) -> str:
        return (self._lib.spf_last_blind_rotate_kernel(self._h) or b"").decode()

    def last_cmux_kernel(self) -> str:
        return (self._lib.spf_last_cmux_kernel(self._h) or b"").decode()

    def lwe_linear_enqueue(self, stream, slot, kind, B, d_lwe_in, d_lwe_out):
        self._ck(self._lib.spf_lwe_linear_enqueue(self._h, stream, int(slot), int(kind), B, d_lwe_in, d_lwe_out))

    def last_lwe_linear_kernel(self) -> str:
        return (self._lib.spf_last_lwe_linear_kernel(self._h) or b"").decode()

    def glwe_poly_linear_enqueue(self, stream, slot, B, d_glwe_in, d_glwe_out):
        self._ck(self._lib.spf_glwe_poly_linear_enqueue(self._h, stream, int(slot), B, d_glwe_in, d_glwe_out))

    def last_glwe_poly_kernel(self) -> str:
        return (self._lib.spf_last_glwe_poly_kernel(self._h) or b"").decode()

    # the device-pointer forms of the GLWE keyswitch, automorphism round and trace; d_glwe_out may be d_glwe_in itself
    def glwe_keyswitch_enqueue(self, stream, slot, B, d_glwe_in, d_glwe_out):
        self._ck(self._lib.spf_glwe_keyswitch_enqueue(self._h, stream, int(slot) & 0xFFFFFFFF, B, d_glwe_in, d_glwe_out))

    def glwe_automorphism_enqueue(self, stream, round, B, d_glwe_in, d_glwe_out):
        self._ck(self._lib.spf_glwe_automorphism_enqueue(self._h, stream, int(round) & 0xFFFFFFFF, B, d_glwe_in, d_glwe_out))

    # the per-item forms on device pointers: `params` a HOST array of B values (one stream per context)
    def _each_dev(self, fn, stream, B, d_in, params, d_out):
        p = np.ascontiguousarray(params, dtype=np.uint64).reshape(-1)
        if p.shape[0] != int(B):
            raise SpfError(-2, f"{int(B)} items but {p.shape[0]} parameters")
        self._ck(fn(self._h, stream, B, d_in, _ptr(p), d_out))

    def sample_extract_l1_each_dev(self, stream, B, d_glwe, idx, d_out):
        self._each_dev(self._lib.spf_sample_extract_l1_each_devptr, stream, B, d_glwe, idx, d_out)

    def glwe_mul_xn_each_dev(self, stream, B, d_in, amounts, d_out):
        self._each_dev(self._lib.spf_glwe_mul_xn_each_devptr, stream, B, d_in, amounts, d_out)

    def glwe_keyswitch_each_dev(self, stream, slots, B, d_glwe_in, d_glwe_out):
        self._each_dev(self._lib.spf_glwe_keyswitch_each_devptr, stream, B, d_glwe_in, slots, d_glwe_out)

    def glwe_automorphism_each_dev(self, stream, rounds, B, d_glwe_in, d_glwe_out):
        self._each_dev(self._lib.spf_glwe_automorphism_each_devptr, stream, B, d_glwe_in, rounds, d_glwe_out)

    def glwe_trace_enqueue(self, stream, B, d_glwe_in, d_glwe_out):
        self._ck(self._lib.spf_glwe_trace_enqueue(self._h, stream, B, d_glwe_in, d_glwe_out))

    def last_glwe_keyswitch_kernel(self) -> str:
        return (self._lib.spf_last_glwe_keyswitch_kernel(self._h) or b"").decode()

    def lwe_ring_pack_enqueue(self, stream, leaf_kind, p, B, d_leaves, d_scratch, scratch_words, d_glwe_out):
        self._ck(self._lib.spf_lwe_ring_pack_enqueue(self._h, stream, int(leaf_kind), int(p), B, d_leaves, d_scratch, int(scratch_words), d_glwe_out))

    def last_lwe_ring_pack_kernel(self) -> str:
        return (self._lib.spf_last_lwe_ring_pack_kernel(self._h) or b"").decode()

    def last_public_functional_keyswitch_kernel(self) -> str:
        return (self._lib.spf_last_public_functional_keyswitch_kernel(self._h) or b"").decode()

    def last_private_functional_keyswitch_kernel(self) -> str:
        return (self._lib.spf_last_private_functional_keyswitch_kernel(self._h) or b"").decode()

    def last_keyswitch_kernel(self) -> str:
        return (self._lib.spf_last_keyswitch_kernel(self._h) or b"").decode()

    def last_kernel_ms(self, kernel: str = "pbs"):
        ms, n = C.c_double(), C.c_int()
        self._ck(self._lib.spf_last_kernel_ms(self._h, kernel.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value


class _GroupLib:
    """the library seen through a group handle: `spf_X` resolves to `spf_group_X` where the group has that entry point, so
    that every host-array method of Engine runs unchanged over the group"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name.startswith("spf_") and not name.startswith("spf_group_"):
            fn = getattr(self._lib, "spf_group_" + name[4:], None)
            if fn is not None:
                return fn
            if name not in ("spf_version",):   # anything else would take the group handle for a context
                raise SpfError(-2, f"{name} has no group form: use group.member(i)")
        return getattr(self._lib, name)


class _MemberEngine(Engine):
    """member i of a group as an Engine (the `_dev` forms, gate graphs, measurement hooks on that device); the context
    belongs to the group"""

    def __init__(self, group: "Group", member: int):
        self._lib = group._raw
        self.params = group.params
        self.device = group.devices[member]
        self._group = group   # keeps the owner alive
        self._h = C.c_void_p(group._raw.spf_group_ctx(group._h, member))
        if not self._h:
            raise SpfError(-2, f"group has no member {member}")

    def close(self):
        self._h = None


class Group(Engine):
    """Every listed GPU behind one handle (`spf_group`): keys replicated inside the library (RCCL broadcast from member 0),
    host batches cut into contiguous ranges of ceil(B / G).  Has every host-array method of Engine; the device-pointer
    forms belong to a member: `group.member(i)`."""

    def __init__(self, params: Params = DEFAULT_128, devices=(0,)):
        self._raw = load_library()
        self._lib = _GroupLib(self._raw)
        self.params = params
        self.devices = [int(d) for d in devices]
        self.device = self.devices[0] if self.devices else -1
        cp = _cparams(params)
        ids = (C.c_int * len(self.devices))(*self.devices)
        h = C.c_void_p()
        st = self._raw.spf_group_create(C.byref(cp), ids, len(self.devices), C.byref(h))
        if st != 0:
            raise SpfError(st, (self._raw.spf_last_error(None) or b"").decode())
        self._h = h

    def _ck(self, st: int):
        if st != 0:
            raise SpfError(st, (self._raw.spf_group_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None):
            self._raw.spf_group_destroy(self._h)
            self._h = None

    def __len__(self):
        return int(self._raw.spf_group_size(self._h))

    def member(self, i: int) -> Engine:
        return _MemberEngine(self, i)

    def replicate_keys(self):
        self._ck(self._raw.spf_group_replicate_keys(self._h))

    def replication_stats(self) -> dict:
        w, ci, b, ws, t = C.c_double(), C.c_double(), C.c_size_t(), C.c_int(), C.c_char_p()
        self._ck(self._raw.spf_group_replication_stats(self._h, C.byref(w), C.byref(ci), C.byref(b), C.byref(ws), C.byref(t)))
        return {"wire_seconds": w.value, "comm_init_seconds": ci.value, "bytes_per_member": b.value,
                "rccl_world_size": ws.value, "transport": (t.value or b"").decode()}

    def set_member_enabled(self, member: int, enabled: bool):
        self._ck(self._raw.spf_group_set_member_enabled(self._h, member, 1 if enabled else 0))

    def members_in_rotation(self) -> int:
        return int(self._raw.spf_group_members_in_rotation(self._h))

    def debug_fail_next(self, member: int, count: int = 1):
        self._ck(self._raw.spf_group_debug_fail_next(self._h, member, count))

    def lwe_linear_slot_shape(self, slot: int):
        """of member 0: `spf_group_load_lwe_linear_weights` loads every member alike"""
        return self.member(0).lwe_linear_slot_shape(slot)

    def glwe_poly_slot_shape(self, slot: int):
        """of member 0: `spf_group_load_glwe_poly_weights` loads every member alike"""
        return self.member(0).glwe_poly_slot_shape(slot)

    def last_glwe_poly_kernel(self) -> str:
        return self.member(0).last_glwe_poly_kernel()

    def glwe_keyswitch_slot_shape(self, slot: int):
        """of member 0: `spf_group_load_glwe_keyswitch_key_std` loads every member alike"""
        return self.member(0).glwe_keyswitch_slot_shape(slot)

    def last_glwe_keyswitch_kernel(self) -> str:
        return self.member(0).last_glwe_keyswitch_kernel()

    def last_lwe_ring_pack_kernel(self) -> str:
        return self.member(0).last_lwe_ring_pack_kernel()

    def run_graphs(self, graphs):
        """`spf_group_run_graphs`: graphs are `spf_amd.FheCircuit`s made over this group; dealt to the members by cost,
        every member's jobs lowered into one graph, all members side by side"""
        arr = (C.c_void_p * len(graphs))(*[g._g for g in graphs])
        self._ck(self._raw.spf_group_run_graphs(self._h, arr, len(graphs)))

    # the per-context hooks have no group form
    def key_blob(self, which):
        raise SpfError(-2, "key blobs belong to a member: group.member(i).key_blob(which)")

    key_blob_commit = key_blob


class Pool:
    """Call-coalescing front end (`spf_pool`): many threads submit single-ciphertext operations and
    block in wait(); a worker thread runs what is pending as one batch.  The synchronous methods
    below are what a per-op caller (the reference's rayon task) would use."""

    def __init__(self, engine: Engine, max_batch: int = 4096, max_wait_us: int = 200):
        self._lib = load_library()
        self.engine = engine
        h = C.c_void_p()
        if isinstance(engine, Group):   # one pool per member, callers dealt across the devices
            st = self._lib.spf_pool_create_group(engine._h, max_batch, max_wait_us, C.byref(h))
        else:
            st = self._lib.spf_pool_create(engine._h, max_batch, max_wait_us, C.byref(h))
        if st != 0:
            raise SpfError(st, "spf_pool_create failed")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.spf_pool_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_max_inflight(self, n: int):
        st = self._lib.spf_pool_set_max_inflight(self._h, n)
        if st != 0:
            raise SpfError(st, "spf_pool_set_max_inflight failed")

    def set_mixed_parameters(self, on: bool = True):
        """`spf_pool_set_mixed_parameters`: SampleExtract / MulXN / GLWE keyswitch / automorphism calls whose parameters differ
        share a batch, run as one launch of the per-item kernels.  Only before the pool's first submit."""
        st = self._lib.spf_pool_set_mixed_parameters(self._h, 1 if on else 0)
        if st != 0:
            raise SpfError(st, "spf_pool_set_mixed_parameters: only before the pool's first submit")

    def submit_keyswitch(self, output: np.ndarray, input: np.ndarray) -> int:
        """asynchronous form: returns the ticket; buffers must stay alive until wait(ticket) returns"""
        t = C.c_uint64()
        x = _in("pool keyswitch", input, np.uint64, self.engine.params.lwe1_words)
        _out("pool keyswitch", output, np.uint64, self.engine.params.lwe0_words)
        st = self._lib.spf_pool_submit_keyswitch(self._h, _ptr(x), _ptr(output), C.byref(t))
        if st != 0:
            raise SpfError(st, "submit failed")
        self._keep = getattr(self, "_keep", {})
        self._keep[t.value] = (x, output)
        return t.value

    def wait(self, ticket: int):
        try:
            self._wait(ticket)
        finally:
            getattr(self, "_keep", {}).pop(ticket, None)

    def _wait(self, ticket):
        st = self._lib.spf_pool_wait(self._h, ticket)
        if st != 0:
            if isinstance(self.engine, Group):
                eng = self.engine.member(min(ticket >> 56, len(self.engine.devices) - 1))
                raise SpfError(st, (self._lib.spf_last_error(eng._h) or b"").decode())
            raise SpfError(st, (self._lib.spf_last_error(self.engine._h) or b"").decode())

    def keyswitch_lwe_l1_lwe_l0(self, output: np.ndarray, input: np.ndarray):
        t = C.c_uint64()
        x = _in("pool keyswitch", input, np.uint64, self.engine.params.lwe1_words)
        _out("pool keyswitch", output, np.uint64, self.engine.params.lwe0_words)
        st = self._lib.spf_pool_submit_keyswitch(self._h, _ptr(x), _ptr(output), C.byref(t))
        if st != 0:
            raise SpfError(st, "submit failed")
        self._wait(t.value)

    def circuit_bootstrap(self, output: np.ndarray, input: np.ndarray):
        t = C.c_uint64()
        x = _in("pool circuit_bootstrap", input, np.uint64, self.engine.params.lwe0_words)
        _out("pool circuit_bootstrap", output, np.complex128, self.engine.params.cbs_ggsw_complex)
        st = self._lib.spf_pool_submit_circuit_bootstrap(self._h, _ptr(x), _ptr(output), C.byref(t))
        if st != 0:
            raise SpfError(st, "submit failed")
        self._wait(t.value)

    def keyswitch_circuit_bootstrap(self, output: np.ndarray, input_l1: np.ndarray):
        t = C.c_uint64()
        x = _in("pool keyswitch_circuit_bootstrap", input_l1, np.uint64, self.engine.params.lwe1_words)
        _out("pool keyswitch_circuit_bootstrap", output, np.complex128, self.engine.params.cbs_ggsw_complex)
        st = self._lib.spf_pool_submit_keyswitch_circuit_bootstrap(self._h, _ptr(x), _ptr(output), C.byref(t))
        if st != 0:
            raise SpfError(st, "submit failed")
        self._wait(t.value)

    def cmux(self, output: np.ndarray, sel: np.ndarray, a: np.ndarray, b: np.ndarray):
        t = C.c_uint64()
        P = self.engine.params
        s_ = _in("pool cmux", sel, np.complex128, P.cbs_ggsw_complex)
        a_, b_ = _in("pool cmux", a, np.uint64, P.glwe_words), _in("pool cmux", b, np.uint64, P.glwe_words)
        _out("pool cmux", output, np.uint64, P.glwe_words)
        st = self._lib.spf_pool_submit_cmux(self._h, _ptr(s_), _ptr(a_), _ptr(b_), _ptr(output), C.byref(t))
        if st != 0:
            raise SpfError(st, "submit failed")
        self._wait(t.value)

    # -- the other FheOp kinds of CircuitProcessor::exec_op (synchronous forms: submit + wait)
    def _run(self, what, fn, *args):
        t = C.c_uint64()
        st = fn(self._h, *args, C.byref(t))
        if st != 0:
            raise SpfError(st, f"pool {what}: submit failed")
        self._wait(t.value)

    def sample_extract_l1(self, output: np.ndarray, glwe: np.ndarray, idx: int):
        P = self.engine.params
        x = _in("pool sample_extract", glwe, np.uint64, P.glwe_words)
        _out("pool sample_extract", output, np.uint64, P.lwe1_words)
        self._run("sample_extract", self._lib.spf_pool_submit_sample_extract, _ptr(x), int(idx), _ptr(output))

    def glwe_not(self, output: np.ndarray, glwe: np.ndarray):
        P = self.engine.params
        x = _in("pool not", glwe, np.uint64, P.glwe_words)
        _out("pool not", output, np.uint64, P.glwe_words)
        self._run("not", self._lib.spf_pool_submit_not, _ptr(x), _ptr(output))

    def glwe_add(self, output: np.ndarray, a: np.ndarray, b: np.ndarray):
        P = self.engine.params
        a_, b_ = _in("pool glwe_add", a, np.uint64, P.glwe_words), _in("pool glwe_add", b, np.uint64, P.glwe_words)
        _out("pool glwe_add", output, np.uint64, P.glwe_words)
        self._run("glwe_add", self._lib.spf_pool_submit_glwe_add, _ptr(a_), _ptr(b_), _ptr(output))

    def mul_xn(self, output: np.ndarray, glwe: np.ndarray, n: int):
        P = self.engine.params
        x = _in("pool mul_xn", glwe, np.uint64, P.glwe_words)
        _out("pool mul_xn", output, np.uint64, P.glwe_words)
        self._run("mul_xn", self._lib.spf_pool_submit_mul_xn, _ptr(x), int(n), _ptr(output))

    def multiply_glwe_ggsw(self, output: np.ndarray, glwe: np.ndarray, ggsw: np.ndarray):
        P = self.engine.params
        g = _in("pool multiply_glwe_ggsw", ggsw, np.complex128, P.cbs_ggsw_complex)
        x = _in("pool multiply_glwe_ggsw", glwe, np.uint64, P.glwe_words)
        _out("pool multiply_glwe_ggsw", output, np.uint64, P.glwe_words)
        self._run("multiply_glwe_ggsw", self._lib.spf_pool_submit_multiply_ggsw_glwe, _ptr(g), _ptr(x), _ptr(output))

    def glev_cmux(self, output: np.ndarray, sel: np.ndarray, a: np.ndarray, b: np.ndarray):
        P = self.engine.params
        n = P.cbs_radix_count * P.glwe_words
        s_ = _in("pool glev_cmux", sel, np.complex128, P.cbs_ggsw_complex)
        a_, b_ = _in("pool glev_cmux", a, np.uint64, n), _in("pool glev_cmux", b, np.uint64, n)
        _out("pool glev_cmux", output, np.uint64, n)
        self._run("glev_cmux", self._lib.spf_pool_submit_glev_cmux, _ptr(s_), _ptr(a_), _ptr(b_), _ptr(output))

    def scheme_switch(self, output: np.ndarray, glev: np.ndarray):
        P = self.engine.params
        x = _in("pool scheme_switch", glev, np.uint64, P.cbs_radix_count * P.glwe_words)
        _out("pool scheme_switch", output, np.complex128, P.cbs_ggsw_complex)
        self._run("scheme_switch", self._lib.spf_pool_submit_scheme_switch, _ptr(x), _ptr(output))

    # -- keyswitch_glwe_to_glwe under the key of `slot`, one round of the trace's loop, trace: one GLWE per call, word-equal to
    # Engine.glwe_keyswitch / glwe_automorphism / glwe_trace.  Calls with different slots or rounds run in different batches unless the pool mixes parameters (set_mixed_parameters); an
    # empty slot or a missing automorphism key is refused at the submit (SPF_ERR_NO_KEY)
    def _run_glwe_ks(self, what, fn, output, glwe, *param):
        P = self.engine.params
        x = _in(f"pool {what}", glwe, np.uint64, P.glwe_words)
        _out(f"pool {what}", output, np.uint64, P.glwe_words)
        t = C.c_uint64()
        self._ck(fn(self._h, *param, _ptr(x), _ptr(output), C.byref(t)), f"pool {what}")
        self._wait(t.value)

    def glwe_keyswitch(self, output: np.ndarray, glwe: np.ndarray, slot: int):
        self._run_glwe_ks("glwe_keyswitch", self._lib.spf_pool_submit_glwe_keyswitch, output, glwe, int(slot) & 0xFFFFFFFF)

    def glwe_automorphism(self, output: np.ndarray, glwe: np.ndarray, round: int):
        self._run_glwe_ks("glwe_automorphism", self._lib.spf_pool_submit_glwe_automorphism, output, glwe, int(round) & 0xFFFFFFFF)

    def glwe_trace(self, output: np.ndarray, glwe: np.ndarray):
        self._run_glwe_ks("glwe_trace", self._lib.spf_pool_submit_glwe_trace, output, glwe)

    def stats(self):
        ops, launches = C.c_uint64(), C.c_uint64()
        self._lib.spf_pool_stats(self._h, C.byref(ops), C.byref(launches))
        return ops.value, launches.value

    def counters(self) -> dict:
        a = (C.c_uint64 * 11)()
        self._ck(self._lib.spf_pool_counters_get(self._h, C.byref(a)), "spf_pool_counters_get")
        return {"ops": a[0], "launches": a[1], "handle_ops": a[2], "handle_launches": a[3], "reclaimed": a[4],
                "bootstrap_launches_by_shape": {"blind_rotate8": a[5], "blind_rotate2p2": a[6], "blind_rotate2p": a[7]},
                "staging_sets": a[8], "value_mallocs": a[9], "stream_concurrency": a[10]}

    # -- device-resident values (spf_value_*): the operands and results of the `_v` submits ---------------------------------
    def _ck(self, st: int, what: str):
        if st != 0:
            eng = self.engine.member(0) if isinstance(self.engine, Group) else self.engine
            raise SpfError(st, f"{what}: " + (self._lib.spf_last_error(eng._h) or b"").decode())

    _VALUE_DTYPE = {3: np.complex128}

    def upload(self, kind: int, array: np.ndarray, member: int = -1) -> "Value":
        P = self.engine.params
        words = {0: P.lwe0_words, 1: P.lwe1_words, 2: P.glwe_words, 3: 2 * P.cbs_ggsw_complex, 4: P.cbs_radix_count * P.glwe_words}[int(kind)]
        a = np.ascontiguousarray(array)
        if a.nbytes != words * 8:
            raise SpfError(1, f"value of kind {int(kind)} must have {words * 8} bytes, got {a.nbytes}")
        h = C.c_void_p()
        self._ck(self._lib.spf_value_upload(self._h, member, int(kind), _ptr(a), C.byref(h)), "spf_value_upload")
        return Value(self, h)

    def _words(self, kind: int) -> int:
        P = self.engine.params
        return {0: P.lwe0_words, 1: P.lwe1_words, 2: P.glwe_words, 3: 2 * P.cbs_ggsw_complex, 4: P.cbs_radix_count * P.glwe_words}[int(kind)]

    def upload_batch(self, kind: int, arrays: np.ndarray, member: int = -1):
        """`spf_value_upload_batch`: arrays is [n, words of the kind]; one block, one copy -> list of n values"""
        a = np.ascontiguousarray(arrays)
        n = a.shape[0]
        if a.nbytes != n * self._words(kind) * 8:
            raise SpfError(1, f"{n} values of kind {int(kind)} must have {n * self._words(kind) * 8} bytes, got {a.nbytes}")
        hs = (C.c_void_p * n)()
        self._ck(self._lib.spf_value_upload_batch(self._h, member, int(kind), n, _ptr(a), hs), "spf_value_upload_batch")
        return [Value(self, C.c_void_p(h)) for h in hs]

    def download_batch(self, values) -> np.ndarray:
        """`spf_value_download_batch`: -> [n, words] (complex128 for GGSW)"""
        i = values[0].info()
        n = len(values)
        dtype = np.complex128 if i["kind"] == 3 else np.uint64
        out = np.empty((n, i["bytes"] // np.dtype(dtype).itemsize), dtype=dtype)
        hs = (C.c_void_p * n)(*[v._h for v in values])
        self._ck(self._lib.spf_value_download_batch(n, hs, _ptr(out)), "spf_value_download_batch")
        return out

    def trivial(self, kind: int, bit: int, member: int = -1) -> "Value":
        h = C.c_void_p()
        self._ck(self._lib.spf_value_trivial(self._h, member, int(kind), int(bit), C.byref(h)), "spf_value_trivial")
        return Value(self, h)

    def copy_to_member(self, value: "Value", member: int) -> "Value":
        h = C.c_void_p()
        self._ck(self._lib.spf_value_copy_to_member(self._h, value._h, member, C.byref(h)), "spf_value_copy_to_member")
        return Value(self, h)

    def submit_v(self, op: int, inputs, param: int = 0):
        """`spf_pool_submit_op_v`: op is a spf_graph_op (spf_amd.FheOp); returns (result value, ticket) — the value is valid
        once wait(ticket) has returned"""
        arr = (C.c_void_p * len(inputs))(*[v._h for v in inputs])
        h, t = C.c_void_p(), C.c_uint64()
        self._ck(self._lib.spf_pool_submit_op_v(self._h, int(op), arr, len(inputs), int(param), C.byref(h), C.byref(t)), "spf_pool_submit_op_v")
        return Value(self, h), t.value

    def push_v(self, op: int, inputs, param: int = 0) -> "Value":
        """`spf_pool_submit_op_v` without a ticket: the operands may be results that are still pending (the pool orders and
        batches what is pushed by level); Value.wait() on the result — or on anything computed from it — makes it run"""
        arr = (C.c_void_p * len(inputs))(*[v._h for v in inputs])
        h = C.c_void_p()
        self._ck(self._lib.spf_pool_submit_op_v(self._h, int(op), arr, len(inputs), int(param), C.byref(h), None), "spf_pool_submit_op_v")
        return Value(self, h)

    def flush(self):
        """`spf_pool_flush`: what has been pushed so far is launched (nothing is waited for)"""
        self._ck(self._lib.spf_pool_flush(self._h), "spf_pool_flush")

    def run_v(self, op: int, inputs, param: int = 0) -> "Value":
        v, t = self.submit_v(op, inputs, param)
        try:
            self._wait(t)
        except SpfError:
            v.release()
            raise
        return v

    # the three GLWE keyswitch operations by handle through their named entry points (run_v / push_v / submit_v with
    # FheOp.GLWE_KEYSWITCH / GLWE_AUTOMORPHISM / GLWE_TRACE take the generic door): wait=False pushes without a ticket — the operand
    # may then be pending, and Value.wait() on the result makes it run
    def _glwe_ks_v(self, name, glwe: "Value", param, wait: bool) -> "Value":
        h, t = C.c_void_p(), C.c_uint64()
        fn = getattr(self._lib, name)
        self._ck(fn(self._h, *param, glwe._h, C.byref(h), C.byref(t) if wait else None), name)
        v = Value(self, h)
        if wait:
            try:
                self._wait(t.value)
            except SpfError:
                v.release()
                raise
        return v

    def glwe_keyswitch_v(self, slot: int, glwe: "Value", wait: bool = True) -> "Value":
        return self._glwe_ks_v("spf_pool_submit_glwe_keyswitch_v", glwe, (int(slot) & 0xFFFFFFFF,), wait)

    def glwe_automorphism_v(self, round: int, glwe: "Value", wait: bool = True) -> "Value":
        return self._glwe_ks_v("spf_pool_submit_glwe_automorphism_v", glwe, (int(round) & 0xFFFFFFFF,), wait)

    def glwe_trace_v(self, glwe: "Value", wait: bool = True) -> "Value":
        return self._glwe_ks_v("spf_pool_submit_glwe_trace_v", glwe, (), wait)

    def keyswitch_circuit_bootstrap_v(self, lwe1: "Value") -> "Value":
        h, t = C.c_void_p(), C.c_uint64()
        self._ck(self._lib.spf_pool_submit_keyswitch_circuit_bootstrap_v(self._h, lwe1._h, C.byref(h), C.byref(t)),
                 "spf_pool_submit_keyswitch_circuit_bootstrap_v")
        v = Value(self, h)
        self._wait(t.value)
        return v

    def _submit_blind_rotation_v(self, glwe: "Value", shift_values, log_stride: int, ticket):
        shift_values = list(shift_values)
        arr = (C.c_void_p * max(len(shift_values), 1))(*[v._h for v in shift_values])
        h = C.c_void_p()
        self._ck(self._lib.spf_pool_submit_blind_rotation_v(self._h, glwe._h, arr, len(shift_values), int(log_stride), C.byref(h), ticket),
                 "spf_pool_submit_blind_rotation_v")
        return Value(self, h)

    def push_blind_rotation_v(self, glwe: "Value", shift_values, log_stride: int = 0) -> "Value":
        """`spf_pool_submit_blind_rotation_v` without a ticket: glwe * X^-(s << log_stride), s given by the GGSW values of its bits
        (bit 0 first); the operands may still be pending, Value.wait() on the result makes the chain run"""
        return self._submit_blind_rotation_v(glwe, shift_values, log_stride, None)

    def blind_rotation_v(self, glwe: "Value", shift_values, log_stride: int = 0) -> "Value":
        """the same, waited for: word-equal to `Engine.blind_rotation` of the downloaded operands"""
        t = C.c_uint64()
        v = self._submit_blind_rotation_v(glwe, shift_values, log_stride, C.byref(t))
        try:
            self._wait(t.value)
        except SpfError:
            v.release()
            raise
        return v

    def value_stats(self) -> dict:
        a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
        self._ck(self._lib.spf_pool_value_stats(self._h, C.byref(a), C.byref(b), C.byref(c)), "spf_pool_value_stats")
        return {"live_values": a.value, "live_bytes": b.value, "cached_bytes": c.value}

    def trim(self):
        self._ck(self._lib.spf_pool_trim(self._h), "spf_pool_trim")


class Value:
    """one device-resident ciphertext (`spf_value`): holds ONE reference, dropped by release() / garbage collection"""

    def __init__(self, pool: Pool, handle):
        self._pool = pool
        self._lib = pool._lib
        self._h = handle

    def info(self) -> dict:
        k, b, m, r = C.c_int(), C.c_size_t(), C.c_int(), C.c_int()
        st = self._lib.spf_value_info(self._h, C.byref(k), C.byref(b), C.byref(m), C.byref(r))
        if st != 0:
            raise SpfError(st, "spf_value_info")
        return {"kind": k.value, "bytes": b.value, "member": m.value, "valid": bool(r.value)}

    def download(self) -> np.ndarray:
        i = self.info()
        out = np.empty(i["bytes"] // (16 if i["kind"] == 3 else 8), dtype=np.complex128 if i["kind"] == 3 else np.uint64)
        st = self._lib.spf_value_download(self._h, _ptr(out))
        if st != 0:
            raise SpfError(st, "spf_value_download: the value is not valid (wait for its ticket first)")
        return out

    def wait(self) -> "Value":
        """`spf_value_wait`: until the operation that produces the value has run"""
        st = self._lib.spf_value_wait(self._h)
        if st != 0:
            raise SpfError(st, "spf_value_wait: the producing operation failed")
        return self

    def device_ptr(self) -> int:
        p = C.c_void_p()
        st = self._lib.spf_value_device_ptr(self._h, C.byref(p))
        if st != 0:
            raise SpfError(st, "spf_value_device_ptr: the value is not valid")
        return p.value

    def release(self):
        if getattr(self, "_h", None):
            self._lib.spf_value_release(self._h)
            self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass
