// spf_ops_launch.hpp — the dispatcher from an operation of the table (spf_ops.hpp) over contiguous operand rows to the `_dev` /
// `pool_*` launchers: the one part of the operation table that needs `spf_ctx`, `Scratch` and a HIP stream.  spf_ops.hpp itself is
// free of HIP, so that the planners and their CPU check programs can include it.
// Included by spf_hip.hip right behind spf_ops.hpp.
#pragma once
#include "spf_ops.hpp"

// ---------------------------------------------------------------- the dispatcher
// (defined further down in spf_hip.hip: a batch of a pool's staging set, on the set's stream and intermediates)
static spf_status pool_keyswitch(spf_ctx* c, hipStream_t s, size_t B, const uint64_t* d_in, uint64_t* d_out, Scratch* sc);
static spf_status pool_circuit_bootstrap(spf_ctx* c, hipStream_t s, size_t B, const uint64_t* d_lwe, double* d_ggsw, Scratch* sc,
                                         int per_wg_hint);
static spf_status launch_lwe_pack(spf_ctx* c, hipStream_t s, size_t B, const uint64_t* d_left, const uint64_t* d_right,
                                  uint32_t plaintext_bits, uint64_t* d_out);
// (GLWE keyswitch, automorphism round, trace over consecutive rows: `mode` a GlweKsMode, `arg` the slot or the round)
static spf_status glwe_ks_enqueue(spf_ctx* c, void* stream, int mode, uint32_t arg, size_t B, const uint64_t* d_in, uint64_t* d_out);
namespace {
spf_status launch_blind_rotate(spf_ctx* c, hipStream_t s, size_t B, const uint64_t* d_lwe, const uint64_t* d_lut, size_t lut_stride,
                               uint32_t log_chi, uint32_t log_v, uint64_t body_rotate, uint64_t* d_out, size_t out_stride, bool extract,
                               int per_wg_hint);
}

namespace spf_ops {

// The kernels of B operations of one kind: operands in[0 .. arity) and `out` are contiguous device rows.  (The CMUX family over
// SCATTERED operands — by handle on the tuned parameter sets, and in gate graphs — goes to spf_cmux_scattered_dev instead.)
//   scr != null: a pool's batch — the staging set's intermediates, the population's workgroup shape (per_wg, launch_blind_rotate),
//                no batch-limit check (a set never holds that many); d_mid = the set's level-0 rows: the keyswitched LWE of
//                OP_GATE_CBS, the packed input of OP_PBS_BIVARIATE (not the context's `packed`: several sets run side by side);
//   scr == null: a gate graph's level — the public `_dev` entry points on the context's own intermediates, with their checks.
// The two bootstraps by table read table row b at in[arity - 1] + b GLWEs, or ONE table for all rows with `one_lut`.
inline spf_status launch_op(spf_ctx* c, hipStream_t s, int op, size_t B, const void* const in[3], void* out, uint64_t param,
                            Scratch* scr, int per_wg, void* d_mid, bool one_lut = false)
{
    const size_t lut_stride = one_lut ? 0 : glwe_words(c->prm);
    const auto u64 = [](const void* p) { return static_cast<const uint64_t*>(p); };
    const auto f64 = [](const void* p) { return static_cast<const double*>(p); };
    const auto keyswitch = [&](const void* lwe1, void* lwe0) {
        return scr ? pool_keyswitch(c, s, B, u64(lwe1), (uint64_t*)lwe0, scr) : spf_keyswitch_lwe_l1_lwe_l0_dev(c, s, B, u64(lwe1), (uint64_t*)lwe0);
    };
    const auto bootstrap = [&](const void* lwe0, void* ggsw) {
        return scr ? pool_circuit_bootstrap(c, s, B, u64(lwe0), (double*)ggsw, scr, per_wg) : spf_circuit_bootstrap_dev(c, s, B, u64(lwe0), (double*)ggsw);
    };
    switch (op) {
    case OP_KEYSWITCH: return keyswitch(in[0], out);
    case OP_CBS: return bootstrap(in[0], out);
    case OP_GATE_CBS: { // FheOp::KeyswitchL1toL0 -> FheOp::CircuitBootstrap, the level-0 LWE stays in HBM
        const spf_status st = keyswitch(in[0], d_mid);
        return st == SPF_OK ? bootstrap(d_mid, out) : st;
    }
    case OP_CMUX: return spf_cmux_dev(c, s, B, f64(in[0]), u64(in[1]), u64(in[2]), (uint64_t*)out);
    case OP_SAMPLE_EXTRACT: return spf_sample_extract_l1_dev(c, s, B, u64(in[0]), (size_t)param, (uint64_t*)out);
    case OP_NOT: return spf_glwe_not_dev(c, s, B, u64(in[0]), (uint64_t*)out);
    case OP_GLWE_ADD: return spf_glwe_xor_dev(c, s, B, u64(in[0]), u64(in[1]), (uint64_t*)out);
    case OP_MUL_XN: return spf_glwe_mul_xn_dev(c, s, B, u64(in[0]), (size_t)param, (uint64_t*)out);
    case OP_MULTIPLY_GGSW_GLWE: return spf_multiply_glwe_ggsw_dev(c, s, B, u64(in[1]), f64(in[0]), (uint64_t*)out);
    case OP_GLEV_CMUX: return spf_glev_cmux_dev(c, s, B, f64(in[0]), u64(in[1]), u64(in[2]), (uint64_t*)out);
    case OP_SCHEME_SWITCH: return spf_scheme_switch_dev(c, s, B, u64(in[0]), (double*)out);
    case OP_PBS_UNIVARIATE:
        if (!scr) return spf_pbs_univariate_dev(c, s, B, u64(in[0]), u64(in[1]), lut_stride, (uint64_t*)out);
        return launch_blind_rotate(c, s, B, u64(in[0]), u64(in[1]), lut_stride, 0, 0, 0, (uint64_t*)out, lwe1_words(c->prm), true, per_wg);
    case OP_PBS_BIVARIATE: {
        if (!scr) return spf_pbs_bivariate_dev(c, s, B, u64(in[0]), u64(in[1]), u64(in[2]), lut_stride, (uint32_t)param, (uint64_t*)out);
        const spf_status st = launch_lwe_pack(c, s, B, u64(in[0]), u64(in[1]), (uint32_t)param, (uint64_t*)d_mid);
        if (st != SPF_OK) return st;
        return launch_blind_rotate(c, s, B, (const uint64_t*)d_mid, u64(in[2]), lut_stride, 0, 0, 0, (uint64_t*)out, lwe1_words(c->prm), true, per_wg);
    }
    // one launch, no intermediates: the same arm for a pool's batch and a graph's level.  (Scattered operands by handle and in gate
    // graphs go to launch_glwe_ks_rows instead: the rows' `rows_in_place`.)
    case OP_GLWE_KEYSWITCH: return glwe_ks_enqueue(c, s, spf::GLWE_KS_KEYSWITCH, (uint32_t)param, B, u64(in[0]), (uint64_t*)out);
    case OP_GLWE_AUTOMORPHISM: return glwe_ks_enqueue(c, s, spf::GLWE_KS_AUTOMORPHISM, (uint32_t)param, B, u64(in[0]), (uint64_t*)out);
    case OP_GLWE_TRACE: return glwe_ks_enqueue(c, s, spf::GLWE_KS_TRACE, 0, B, u64(in[0]), (uint64_t*)out);
    case OP_ROT_CMUX: return fail(c, SPF_ERR_INVALID_ARGUMENT, "a rotate-CMUX step reads its operands through a pointer table only");
    default: return fail(c, SPF_ERR_INVALID_ARGUMENT, "unknown graph operation");
    }
}

} // namespace spf_ops
