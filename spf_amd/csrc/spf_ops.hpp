// spf_ops.hpp — the host-side facts about ciphertext kinds and operations, stated once.
//
// The library runs the ten `FheOp` kinds of `CircuitProcessor::exec_op` (circuit_processor/mod.rs:255-540) through the gate graph,
// the pool by host pointer, the pool by handle and the device group.  Everything those routes have to agree on lives here:
//   * the size of a ciphertext of each spf_value_kind (value_words / value_bytes over the four word helpers);
//   * the shape of a batch — words per item of each operand and of the result, the batch limit — that the device-pointer, the
//     host-pointer and the group form of an entry point share (BatchShape: one function per family; spf_ops::shape for the table);
//   * ONE table row per operation: the spf_graph_op it answers to, arity, operand kinds, result kind, the scheduling flags and
//     the rule for its parameter — an operation is DECLARED by adding its row (and its arm in launch_op);
//   * the parameter rule as a function (op_param).
// The dispatcher from an operation over contiguous operand rows to the `_dev` / `pool_*` launchers (launch_op) is
// spf_ops_launch.hpp: it needs `spf_ctx` and a stream.  This header is free of HIP: spf_graph_plan.hpp and its CPU check program
// include it.  Included by spf_hip.hip behind `Scratch`, `spf_ctx` and `fail`, ahead of spf_values.hpp / spf_pool.hpp.
#pragma once
#include "../../include/spf_hip.h"

#include <cstddef>
#include <cstdint>
#include <cstdio>

// ---------------------------------------------------------------- sizes (the only formulas)
inline size_t lwe0_words(const spf_params& p) { return (size_t)p.lwe_dimension + 1; }
inline size_t lwe1_words(const spf_params& p) { return (size_t)p.glwe_size * p.polynomial_degree + 1; }
inline size_t glwe_words(const spf_params& p) { return (size_t)(p.glwe_size + 1) * p.polynomial_degree; }
inline size_t ggsw_fft_complex(const spf_params& p, uint32_t count)
{
    return (size_t)(p.glwe_size + 1) * count * (p.glwe_size + 1) * (p.polynomial_degree / 2);
}

// 64-bit words of one ciphertext of `kind` as it lies in memory (a complex f64 of a GGSW spectrum is two); 0 = unknown kind
inline size_t value_words(const spf_params& p, int kind)
{
    switch (kind) {
    case SPF_VAL_LWE0: return lwe0_words(p);
    case SPF_VAL_LWE1: return lwe1_words(p);
    case SPF_VAL_GLWE1: return glwe_words(p);
    case SPF_VAL_GGSW1: return 2 * ggsw_fft_complex(p, p.cbs_radix_count);
    case SPF_VAL_GLEV1: return (size_t)p.cbs_radix_count * glwe_words(p);
    default: return 0;
    }
}
inline size_t value_bytes(const spf_params& p, int kind) { return 8 * value_words(p, kind); }

// ---------------------------------------------------------------- batch shapes
// What the three forms of a batched entry point (device pointers, host pointers, group) have to agree on: the 64-bit words ONE item
// of each operand and of the result occupies, and the largest batch.  One function per family of entry points, from spf_params and
// the plain numbers the family depends on (no spf_ctx: the context-level checks in spf_hip.hip read those numbers under its lock).
struct BatchShape {
    int n_in;
    size_t in_words[3];
    size_t out_words;
    size_t max_batch;
};
constexpr size_t kBatchMax = 0x7fffffff;     // one launch of a kernel that takes one unit per item
constexpr size_t kBatchMaxRows = 0x0fffffff; // ... that takes several units or rows per item: the limit is on items * rows

// every operand and the result one ciphertext of a spf_value_kind per item
inline BatchShape kinds_shape(const spf_params& p, size_t max_batch, int out, int in0, int in1 = -1, int in2 = -1)
{
    return {in2 >= 0 ? 3 : in1 >= 0 ? 2 : 1, {value_words(p, in0), value_words(p, in1), value_words(p, in2)}, value_words(p, out), max_batch};
}
// the forward transform: one polynomial of N words into its N/2 complex bins
inline BatchShape poly_fft_shape(const spf_params& p) { return {1, {p.polynomial_degree, 0, 0}, p.polynomial_degree, kBatchMax}; }
// the bootstraps by a lookup table: one or two level-0 LWEs in, a GLWE or its sample extract out; the table is the last operand and
// advances by the caller's lut_stride (0: one table for the batch — what it occupies in all is the host form's to work out)
inline BatchShape pbs_shape(const spf_params& p, bool extract, bool bivariate = false, size_t lut_stride = 0)
{
    BatchShape sh = kinds_shape(p, kBatchMax, extract ? SPF_VAL_LWE1 : SPF_VAL_GLWE1, SPF_VAL_LWE0, bivariate ? SPF_VAL_LWE0 : -1);
    sh.in_words[sh.n_in++] = lut_stride;
    return sh;
}
// (an operation of the table below: spf_ops::shape)
// the two stages of a circuit bootstrap that are no operation of the table: lo-noise GLWE -> GLEV, and the fused gate LWE1 -> GLWE
inline BatchShape trace_shape(const spf_params& p) { return kinds_shape(p, kBatchMaxRows, SPF_VAL_GLEV1, SPF_VAL_GLWE1); }
inline BatchShape gate_bootstrap_shape(const spf_params& p) { return kinds_shape(p, kBatchMax, SPF_VAL_GLWE1, SPF_VAL_LWE1); }
// packed integers: n_bits ciphertexts of `in` per item into one of `out` (pack), or one of `in` into n_bits of `out` (the unpacks)
inline BatchShape packed_shape(const spf_params& p, size_t n_bits, int in, int out, bool pack)
{
    return {1, {value_words(p, in) * (pack ? n_bits : 1), 0, 0}, value_words(p, out) * (pack ? 1 : n_bits), n_bits ? kBatchMaxRows / n_bits : 0};
}
// blind rotation by an encrypted shift: an item's n_bits selectors, then its GLWE
inline BatchShape blind_rotation_shape(const spf_params& p, size_t n_bits)
{
    return {2, {n_bits * value_words(p, SPF_VAL_GGSW1), glwe_words(p), 0}, glwe_words(p), n_bits ? kBatchMaxRows / n_bits : 0};
}
// public functional keyswitch: lwe_count rows of the key's from_dimension + 1 words into one GLWE
inline BatchShape pufks_shape(const spf_params& p, size_t lwe_count, size_t from_dimension)
{
    return {1, {lwe_count * (from_dimension + 1), 0, 0}, glwe_words(p), lwe_count ? kBatchMaxRows / lwe_count : 0};
}
// private functional keyswitch: one row of the keys' lwe_count * (from_dimension + 1) words into one GLWE; the GGSW components:
// cbs_radix_count such rows into one integer-form GGSW (as many words as its spectrum)
inline BatchShape pfks_shape(const spf_params& p, size_t row_words) { return {1, {row_words, 0, 0}, glwe_words(p), kBatchMaxRows}; }
inline BatchShape pfks_components_shape(const spf_params& p, size_t row_words)
{
    return {1, {p.cbs_radix_count * row_words, 0, 0}, value_words(p, SPF_VAL_GGSW1), p.cbs_radix_count ? kBatchMaxRows / p.cbs_radix_count : 0};
}
inline BatchShape cbs_via_pfks_shape(const spf_params& p)
{
    return kinds_shape(p, p.cbs_radix_count ? kBatchMaxRows / p.cbs_radix_count : 0, SPF_VAL_GGSW1, SPF_VAL_LWE0);
}
// plaintext linear maps: K ciphertexts of `kind` (a level-0 or level-1 LWE) into M
inline BatchShape lwe_linear_batch_shape(const spf_params& p, size_t M, size_t K, int kind)
{
    return {1, {K * value_words(p, kind), 0, 0}, M * value_words(p, kind), kBatchMaxRows / (M > K ? M : K ? K : 1)};
}
// plaintext polynomial linear maps: K GLWEs into M
inline BatchShape glwe_poly_batch_shape(const spf_params& p, size_t M, size_t K)
{
    return {1, {K * glwe_words(p), 0, 0}, M * glwe_words(p), kBatchMaxRows / (M > K ? M : K ? K : 1)};
}
// GLWE keyswitch, one automorphism round and the trace: one GLWE in, one GLWE out, one unit per item
inline BatchShape glwe_ks_shape(const spf_params& p) { return kinds_shape(p, kBatchMax, SPF_VAL_GLWE1, SPF_VAL_GLWE1); }

// ---------------------------------------------------------------- the operation table
namespace spf_ops {

// The pool's numbering: one kind per `FheOp` that `exec_op` hands to `Evaluation`, plus the KeyswitchL1toL0 -> CircuitBootstrap
// chain, plus one step of a blind rotation by an encrypted shift (OP_ROT_CMUX: spf_pool_submit_blind_rotation_v pushes one per bit;
// in gate graphs the same step is a node of spf_graph_add_blind_rotation).  The pool's lanes, the SPF_POOL_TRACE lines and tools/pool_trace_phases.py carry these numbers.
enum Op {
    OP_KEYSWITCH = 0, OP_CBS = 1, OP_CMUX = 2, OP_GATE_CBS = 3,
    OP_SAMPLE_EXTRACT = 4, OP_NOT = 5, OP_GLWE_ADD = 6, OP_MUL_XN = 7, OP_MULTIPLY_GGSW_GLWE = 8, OP_GLEV_CMUX = 9, OP_SCHEME_SWITCH = 10,
    OP_ROT_CMUX = 11,
    // the bootstraps by a caller's lookup table (programmable_bootstrap_univariate / _bivariate), the table an operand
    OP_PBS_UNIVARIATE = 12, OP_PBS_BIVARIATE = 13,
    // `keyswitch_glwe_to_glwe`, one round of the trace's loop and `trace` (spf_glwe_keyswitch.hpp): the parameter is the
    // keyswitch-key slot / the round / nothing
    OP_GLWE_KEYSWITCH = 14, OP_GLWE_AUTOMORPHISM = 15, OP_GLWE_TRACE = 16,
    N_OPS = 17
};

enum ParamRule {
    PARAM_NONE, PARAM_INDEX_BELOW_N, PARAM_AMOUNT_MOD_2N, PARAM_ROTATION_BELOW_N, PARAM_PLAINTEXT_BITS_BELOW_64,
    PARAM_GLWE_KSK_SLOT, PARAM_ROUND_1_TO_LOG_N
};
constexpr int kNone = -1; // no spf_graph_op / no operand in this slot

struct OpRow {
    int op;           // its own index (checked below: the rows stand in the enum's order)
    int graph_op;     // the spf_graph_op it answers to, or kNone
    int arity;
    int in_kind[3];   // spf_value_kind per operand, in the order spf_graph_add_op takes them; kNone beyond the arity
    int out_kind;
    bool cmux_family; // read scattered operands in place through a pointer table (spf_cmux_scattered_dev)
    bool heavy;       // milliseconds on the GPU: caller groups, pacing and the "previous batch still out" rule apply (spf_pool.hpp)
    ParamRule param;
    // By handle and in gate graphs the operands are read where they lie, through a table of ONE pointer per item, by
    // launch_glwe_ks_rows; the output stays one block of consecutive rows that the launcher passes beside the table (and that
    // overlaps no operand).  Not cmux_family: that table carries four pointers per unit — selector, low, high AND the output —
    // so its units may be sorted and its outputs scattered; here item i of the table is row i of the output.
    bool rows_in_place = false;
};

constexpr OpRow kOps[N_OPS] = {
    {OP_KEYSWITCH, SPF_OP_KEYSWITCH_L1_TO_L0, 1, {SPF_VAL_LWE1, kNone, kNone}, SPF_VAL_LWE0, false, false, PARAM_NONE},
    {OP_CBS, SPF_OP_CIRCUIT_BOOTSTRAP, 1, {SPF_VAL_LWE0, kNone, kNone}, SPF_VAL_GGSW1, false, true, PARAM_NONE},
    {OP_CMUX, SPF_OP_CMUX, 3, {SPF_VAL_GGSW1, SPF_VAL_GLWE1, SPF_VAL_GLWE1}, SPF_VAL_GLWE1, true, false, PARAM_NONE},
    {OP_GATE_CBS, kNone, 1, {SPF_VAL_LWE1, kNone, kNone}, SPF_VAL_GGSW1, false, true, PARAM_NONE},
    {OP_SAMPLE_EXTRACT, SPF_OP_SAMPLE_EXTRACT, 1, {SPF_VAL_GLWE1, kNone, kNone}, SPF_VAL_LWE1, false, false, PARAM_INDEX_BELOW_N},
    {OP_NOT, SPF_OP_NOT, 1, {SPF_VAL_GLWE1, kNone, kNone}, SPF_VAL_GLWE1, false, false, PARAM_NONE},
    {OP_GLWE_ADD, SPF_OP_GLWE_ADD, 2, {SPF_VAL_GLWE1, SPF_VAL_GLWE1, kNone}, SPF_VAL_GLWE1, false, false, PARAM_NONE},
    {OP_MUL_XN, SPF_OP_MUL_XN, 1, {SPF_VAL_GLWE1, kNone, kNone}, SPF_VAL_GLWE1, false, false, PARAM_AMOUNT_MOD_2N},
    {OP_MULTIPLY_GGSW_GLWE, SPF_OP_MULTIPLY_GGSW_GLWE, 2, {SPF_VAL_GGSW1, SPF_VAL_GLWE1, kNone}, SPF_VAL_GLWE1, true, false, PARAM_NONE},
    {OP_GLEV_CMUX, SPF_OP_GLEV_CMUX, 3, {SPF_VAL_GGSW1, SPF_VAL_GLEV1, SPF_VAL_GLEV1}, SPF_VAL_GLEV1, true, false, PARAM_NONE},
    {OP_SCHEME_SWITCH, SPF_OP_SCHEME_SWITCH, 1, {SPF_VAL_GLEV1, kNone, kNone}, SPF_VAL_GGSW1, false, false, PARAM_NONE},
    // out = cmux(selector, acc, X^-param * acc): the high operand is a rotated read of the low one (launch_cmux_rot_scattered)
    {OP_ROT_CMUX, kNone, 2, {SPF_VAL_GGSW1, SPF_VAL_GLWE1, kNone}, SPF_VAL_GLWE1, true, false, PARAM_ROTATION_BELOW_N},
    // out = sample_extract(blind rotation of the table by the LWE), the table the LAST operand; bivariate: by left * 2^param + right
    {OP_PBS_UNIVARIATE, SPF_OP_PBS_UNIVARIATE, 2, {SPF_VAL_LWE0, SPF_VAL_GLWE1, kNone}, SPF_VAL_LWE1, false, true, PARAM_NONE},
    {OP_PBS_BIVARIATE, SPF_OP_PBS_BIVARIATE, 3, {SPF_VAL_LWE0, SPF_VAL_LWE0, SPF_VAL_GLWE1}, SPF_VAL_LWE1, false, true, PARAM_PLAINTEXT_BITS_BELOW_64},
    // out = keyswitch(in, slot param) / keyswitch(in(X^t), automorphism key of round param) / trace(in): one launch per batch,
    // microseconds (the trace: 0.024 ms a round at B = 256, profiles/r32_glwe_keyswitch.md; by handle: profiles/r34_glwe_keyswitch_pool.md)
    {OP_GLWE_KEYSWITCH, SPF_OP_GLWE_KEYSWITCH, 1, {SPF_VAL_GLWE1, kNone, kNone}, SPF_VAL_GLWE1, false, false, PARAM_GLWE_KSK_SLOT, true},
    {OP_GLWE_AUTOMORPHISM, SPF_OP_GLWE_AUTOMORPHISM, 1, {SPF_VAL_GLWE1, kNone, kNone}, SPF_VAL_GLWE1, false, false, PARAM_ROUND_1_TO_LOG_N, true},
    {OP_GLWE_TRACE, SPF_OP_GLWE_TRACE, 1, {SPF_VAL_GLWE1, kNone, kNone}, SPF_VAL_GLWE1, false, false, PARAM_NONE, true},
};

constexpr const OpRow& row(int op) { return kOps[op]; } // op: a valid pool operation
constexpr bool heavy(int op) { return kOps[op].heavy; }
constexpr bool cmux_family(int op) { return kOps[op].cmux_family; }
constexpr bool rows_in_place(int op) { return kOps[op].rows_in_place; }
// the pool operation a spf_graph_op stands for; kNone for a value that is none of the fifteen
constexpr int pool_op_of(int graph_op)
{
    for (int op = 0; op < N_OPS; op++)
        if (graph_op != kNone && kOps[op].graph_op == graph_op) return op;
    return kNone;
}

inline void in_out_bytes(const spf_params& p, int op, size_t (&in)[3], size_t& out)
{
    for (int k = 0; k < 3; k++) in[k] = value_bytes(p, kOps[op].in_kind[k]); // (kNone: 0 bytes)
    out = value_bytes(p, kOps[op].out_kind);
}

// the batch shape of the entry points that run operation `op`: its row's kinds, operands in the row's order; an operation that
// ends in the circuit-bootstrap tail (a GGSW out) launches cbs_radix_count units per item
inline BatchShape shape(const spf_params& p, int op)
{
    const OpRow& r = kOps[op];
    return kinds_shape(p, r.out_kind == SPF_VAL_GGSW1 ? kBatchMaxRows : kBatchMax, r.out_kind, r.in_kind[0], r.in_kind[1], r.in_kind[2]);
}

// the per-item forms of a parameterised single-operand operation (spf_*_each_*: OP_SAMPLE_EXTRACT, OP_MUL_XN, OP_GLWE_KEYSWITCH,
// OP_GLWE_AUTOMORPHISM): the operation's own shape with the parameters as a second operand of ONE word per item.  That operand is
// a HOST array in every form (it is read during the call and never staged: host_batch gets the first operand alone); it stands in
// the shape so that the group form deals it in the same contiguous shards as the items.
inline BatchShape each_shape(const spf_params& p, int op)
{
    BatchShape sh = shape(p, op);
    sh.in_words[sh.n_in++] = 1;
    return sh;
}
constexpr bool has_each_form(int op) { return op == OP_SAMPLE_EXTRACT || op == OP_MUL_XN || op == OP_GLWE_KEYSWITCH || op == OP_GLWE_AUTOMORPHISM; }

// The parameter of an operation, as every entry point takes it: a SampleExtract index must be below N (`why` says so), a MulXN
// amount is reduced mod 2N, a rotate-CMUX rotation lies in 1 .. N - 1,
// a bivariate bootstrap's plaintext_bits are below 64, a GLWE keyswitch's slot is below SPF_GLWE_KSK_SLOTS, an automorphism's round
// lies in 1 .. log2 N (both texts carry the number, in a buffer of the calling thread: read `why` before the thread's next call),
// every other operation's parameter — the trace's too — is 0 whatever the caller passed.
inline uint32_t log2_degree(const spf_params& p)
{
    uint32_t log_n = 0;
    while (((uint64_t)1 << (log_n + 1)) <= p.polynomial_degree) log_n++;
    return log_n;
}
inline spf_status op_param(const spf_params& p, int op, uint64_t* param, const char** why)
{
    static thread_local char text[96];
    switch (kOps[op].param) {
    case PARAM_GLWE_KSK_SLOT:
        if (*param < SPF_GLWE_KSK_SLOTS) return SPF_OK;
        std::snprintf(text, sizeof text, "slot %llu >= SPF_GLWE_KSK_SLOTS = %d", (unsigned long long)*param, (int)SPF_GLWE_KSK_SLOTS);
        *why = text;
        return SPF_ERR_INVALID_ARGUMENT;
    case PARAM_ROUND_1_TO_LOG_N:
        if (*param >= 1 && *param <= log2_degree(p)) return SPF_OK;
        std::snprintf(text, sizeof text, "round %llu outside 1 .. log2 N = %u", (unsigned long long)*param, log2_degree(p));
        *why = text;
        return SPF_ERR_INVALID_ARGUMENT;
    case PARAM_INDEX_BELOW_N:
        if (*param < p.polynomial_degree) return SPF_OK;
        *why = "sample_extract index >= polynomial_degree";
        return SPF_ERR_INVALID_ARGUMENT;
    case PARAM_AMOUNT_MOD_2N: *param %= 2 * (uint64_t)p.polynomial_degree; return SPF_OK;
    case PARAM_ROTATION_BELOW_N:
        if (*param > 0 && *param < p.polynomial_degree) return SPF_OK;
        *why = "rotation must be in 1 .. polynomial_degree - 1";
        return SPF_ERR_INVALID_ARGUMENT;
    case PARAM_PLAINTEXT_BITS_BELOW_64:
        if (*param < 64) return SPF_OK;
        *why = "plaintext_bits must be below 64";
        return SPF_ERR_INVALID_ARGUMENT;
    default: *param = 0; return SPF_OK;
    }
}

namespace check {
constexpr bool is_kind(int k) { return k >= SPF_VAL_LWE0 && k <= SPF_VAL_GLEV1; }
constexpr bool row_ok(const OpRow& r, int index)
{
    if (r.op != index || r.arity < 1 || r.arity > 3 || !is_kind(r.out_kind)) return false;
    for (int k = 0; k < 3; k++)
        if (k < r.arity ? !is_kind(r.in_kind[k]) : r.in_kind[k] != kNone) return false;
    return true;
}
// a row read through the one-pointer table has one operand, and is not of the CMUX family (whose table is another)
constexpr bool rows_ok()
{
    for (int op = 0; op < N_OPS; op++)
        if (!row_ok(kOps[op], op) || (kOps[op].rows_in_place && (kOps[op].arity != 1 || kOps[op].cmux_family))) return false;
    return true;
}
constexpr bool graph_ops_ok() // the fifteen public values name fifteen rows (distinct: each row names its value back), OP_GATE_CBS and OP_ROT_CMUX have none
{
    for (int g = SPF_OP_SAMPLE_EXTRACT; g <= SPF_OP_GLWE_TRACE; g++)
        if (pool_op_of(g) == kNone) return false;
    for (int op = 0; op < N_OPS; op++) {
        const int g = kOps[op].graph_op;
        if (op == OP_GATE_CBS || op == OP_ROT_CMUX ? g != kNone : (g < SPF_OP_SAMPLE_EXTRACT || g > SPF_OP_GLWE_TRACE || pool_op_of(g) != op)) return false;
    }
    return true;
}
static_assert(rows_ok(), "a row is out of the enum's order, or its arity and its operand kinds disagree, or a kind is no spf_value_kind, or a rows_in_place row has more than one operand or is of the CMUX family");
static_assert(graph_ops_ok(), "every spf_graph_op, SPF_OP_SAMPLE_EXTRACT .. SPF_OP_GLWE_TRACE, needs exactly one row, and only OP_GATE_CBS and OP_ROT_CMUX go without a spf_graph_op");
} // namespace check

} // namespace spf_ops
