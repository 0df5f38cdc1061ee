"""Host-side mirror of ``parasol_runtime::Evaluation`` / ``KeylessEvaluation``
(parasol_runtime/src/crypto/evaluation.rs:26-266) for the bootstrap path.

Method names, argument order and meaning follow the reference: the caller allocates ``output``
and the method writes into it (the reference takes ``&mut`` outputs and returns nothing).
Inputs may be single ciphertexts (1-D arrays, as the reference's typed newtypes) or batches
(2-D, leading dimension = batch): the engine underneath is batch-native.  All compute happens in
the HIP library; nothing here touches ciphertext words.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._ffi import Engine
from .params import Params, DEFAULT_128


@dataclass
class ComputeKey:
    """``parasol_runtime::ComputeKey`` (crypto/keys.rs:306-318): the fields this path uses."""

    bs_key: np.ndarray   # BootstrapKeyFft<Complex<f64>>, complex128, reference layout
    ks_key: np.ndarray   # LweKeyswitchKey<u64>
    auto_key: np.ndarray = None  # AutomorphismKeyFft<Complex<f64>>
    ss_key: np.ndarray = None    # SchemeSwitchKeyFft<Complex<f64>>


class Evaluation:
    def __init__(self, compute_key: ComputeKey, params: Params = DEFAULT_128, device: int = 0):
        # Evaluation::new (evaluation.rs:161-197): load the keys; the two circuit bootstraps that give
        # l1ggsw_zero / l1ggsw_one run on the GPU at first use (they need all of bs / auto / ss keys)
        self.params = params
        self.engine = Engine(params, device)
        self.engine.load_bootstrap_key(compute_key.bs_key)
        if compute_key.ks_key is not None and np.size(compute_key.ks_key):
            self.engine.load_keyswitch_key(compute_key.ks_key)
        if compute_key.auto_key is not None:
            self.engine.load_automorphism_key(compute_key.auto_key)
        if compute_key.ss_key is not None:
            self.engine.load_scheme_switch_key(compute_key.ss_key)

    # Evaluation::l1ggsw_zero / l1ggsw_one (evaluation.rs:254-262)
    def l1ggsw_zero(self) -> np.ndarray:
        return self.engine.l1ggsw_constant(0)

    def l1ggsw_one(self) -> np.ndarray:
        return self.engine.l1ggsw_constant(1)

    @staticmethod
    def _store(output: np.ndarray, result: np.ndarray):
        if output.dtype != np.uint64:
            raise TypeError("output must be uint64")
        output[...] = result.reshape(output.shape)

    # KeylessEvaluation::not (evaluation.rs:47-50); `not` is a Python keyword, hence the underscore
    def not_(self, output: np.ndarray, input: np.ndarray):
        self._store(output, self.engine.glwe_not(input))

    # KeylessEvaluation::xor (evaluation.rs:52-55)
    def xor(self, output: np.ndarray, a: np.ndarray, b: np.ndarray):
        self._store(output, self.engine.glwe_xor(a, b))

    # KeylessEvaluation::mul_xn (evaluation.rs:57-65)
    def mul_xn(self, output: np.ndarray, input: np.ndarray, n: int):
        self._store(output, self.engine.glwe_mul_xn(input, n))

    # KeylessEvaluation::sample_extract_l1 (evaluation.rs:126-133)
    def sample_extract_l1(self, output: np.ndarray, input: np.ndarray, idx: int):
        self._store(output, self.engine.sample_extract_l1(input, idx))

    # Evaluation::keyswitch_lwe_l1_lwe_l0 (evaluation.rs:246-255)
    def keyswitch_lwe_l1_lwe_l0(self, output: np.ndarray, input: np.ndarray):
        self._store(output, self.engine.keyswitch_lwe_l1_lwe_l0(input))

    # Evaluation::circuit_bootstrap (evaluation.rs:211-226): L0 LWE -> L1 GGSW (FFT domain)
    def circuit_bootstrap(self, output: np.ndarray, input: np.ndarray):
        if output.dtype != np.complex128:
            raise TypeError("an L1 GGSW ciphertext is complex128 (FFT domain)")
        output[...] = self.engine.circuit_bootstrap(input).reshape(output.shape)

    # Evaluation::scheme_switch (evaluation.rs:231-240): L1 GLEV -> L1 GGSW
    def scheme_switch(self, output: np.ndarray, input: np.ndarray):
        output[...] = self.engine.scheme_switch(input).reshape(output.shape)

    # the bootstrap stage of Evaluation::circuit_bootstrap (evaluation.rs:211-226):
    # hi_noise_lwe_to_lo_noise_glwe (circuit_bootstrapping.rs:387-427).  Output: L1 GLWE whose
    # first cbs_radix.count coefficients hold the gadget levels of the input bit.
    def circuit_bootstrap_pbs(self, output: np.ndarray, input: np.ndarray):
        self._store(output, self.engine.circuit_bootstrap_pbs(input))

    # sunscreen_tfhe::ops::bootstrapping::programmable_bootstrap_univariate
    # (programmable_bootstrapping.rs:291-318)
    def programmable_bootstrap_univariate(self, output: np.ndarray, input: np.ndarray, lut: np.ndarray):
        self._store(output, self.engine.pbs_univariate(input, lut))

    # sunscreen_tfhe::ops::bootstrapping::programmable_bootstrap_bivariate
    # (programmable_bootstrapping.rs:575-621); `lut` from spf_amd.generate_bivariate_lut
    def programmable_bootstrap_bivariate(self, output: np.ndarray, left: np.ndarray, right: np.ndarray, lut: np.ndarray,
                                         plaintext_bits: int):
        self._store(output, self.engine.pbs_bivariate(left, right, lut, plaintext_bits))

    # plaintext linear maps: scalar_mul_ciphertext_mad + add_lwe_inplace (sunscreen_tfhe ops/ciphertext/
    # lwe_ciphertext_ops.rs:48-66, :4-18) for an (M, K) int64 matrix and an optional bias, kept in a slot of the engine:
    # (B, K, W) LWEs of one kind -> (B, M, W)
    def load_lwe_linear_weights(self, slot: int, weights: np.ndarray, bias=None):
        self.engine.load_lwe_linear_weights(slot, weights, bias)

    def lwe_linear(self, output: np.ndarray, input: np.ndarray, slot: int, kind: int = 0):
        self._store(output, self.engine.lwe_linear(slot, input, kind))

    # `glwe_polynomial_mad`, `glwe_scalar_mad`, `sub_glwe_ciphertexts`, `glwe_negate_inplace`, `glwe_rotate`
    # (ops/ciphertext/glwe_ciphertext_ops.rs:164-183, :189-202, :121-141, :147-156, :285-305) as one plaintext polynomial matrix
    def load_glwe_poly_weights(self, slot: int, w, bias=None, shape=None):
        self.engine.load_glwe_poly_weights(slot, w, bias, shape)

    def glwe_poly_linear(self, output: np.ndarray, input: np.ndarray, slot: int):
        self._store(output, self.engine.glwe_poly_linear(slot, input))

    # `keyswitch_glwe_to_glwe` (ops/fft_ops.rs:457-495) under the key of slot `slot` (load_glwe_keyswitch_key_std) and `trace`
    # (ops/automorphisms/mod.rs:53-85) under the automorphism key: (B, k+1, N) GLWEs -> (B, k+1, N)
    def load_glwe_keyswitch_key_std(self, slot: int, key: np.ndarray, radix_log: int, radix_count: int):
        self.engine.load_glwe_keyswitch_key_std(slot, key, radix_log, radix_count)

    def keyswitch_glwe_to_glwe(self, output: np.ndarray, input: np.ndarray, slot: int):
        self._store(output, self.engine.glwe_keyswitch(slot, input))

    def trace(self, output: np.ndarray, input: np.ndarray):
        self._store(output, self.engine.glwe_trace(input))

    # ring packing (spf_lwe_ring_pack_batch; PackLWEs): (B, p, leaf words) LWE1 (leaf_kind 1) or GLWE1 (2) leaves -> (B, k+1, N)
    # under the automorphism key, leaf j's message at coefficient j * N / p (spf_amd.packed.strided_positions)
    def lwe_ring_pack(self, output: np.ndarray, leaves: np.ndarray, p: int, leaf_kind: int = 1):
        self._store(output, self.engine.lwe_ring_pack(leaves, p, leaf_kind))

    # one round (1 .. log2 N) of the trace's loop (ops/automorphisms/mod.rs:72-83).  The three as single-ciphertext operations of
    # a pool, by host pointer or on device-resident values: Pool.glwe_keyswitch / glwe_automorphism / glwe_trace and their `_v`
    # forms (FheOp.GLWE_KEYSWITCH / GLWE_AUTOMORPHISM / GLWE_TRACE through Pool.run_v / push_v)
    def glwe_automorphism(self, output: np.ndarray, input: np.ndarray, round: int):
        self._store(output, self.engine.glwe_automorphism(round, input))

    # generalized_programmable_bootstrap (programmable_bootstrapping.rs:342-410)
    def generalized_programmable_bootstrap(self, output, input, lut, log_chi: int, log_v: int):
        self._store(output, self.engine.generalized_pbs(input, lut, log_chi, log_v, 0))

    # KeylessEvaluation::cmux (evaluation.rs:68-83)
    def cmux(self, output: np.ndarray, sel: np.ndarray, a: np.ndarray, b: np.ndarray):
        self._store(output, self.engine.cmux(sel, a, b))

    # KeylessEvaluation::glev_cmux (evaluation.rs:86-101): L1 GLEV = cbs_radix.count consecutive GLWEs
    def glev_cmux(self, output: np.ndarray, sel: np.ndarray, a: np.ndarray, b: np.ndarray):
        self._store(output, self.engine.glev_cmux(sel, a, b))

    # KeylessEvaluation::multiply_glwe_ggsw (evaluation.rs:104-123)
    def multiply_glwe_ggsw(self, output: np.ndarray, glwe: np.ndarray, ggsw: np.ndarray):
        self._store(output, self.engine.multiply_glwe_ggsw(glwe, ggsw))

    # FheOp::KeyswitchL1toL0 -> FheOp::CircuitBootstrap fused (circuit_processor/mod.rs:329-340,453-463)
    def gate_bootstrap(self, output: np.ndarray, input_l1: np.ndarray):
        self._store(output, self.engine.gate_bootstrap(input_l1))
