// fuzz_host.cpp — mutation fuzz of the library's HOST code under AddressSanitizer + UndefinedBehaviorSanitizer (no GPU).
//
// the untrusted-bytes parsers and the graph builder had never run under a sanitizer.  GPU ASan / XNACK
// are not available on this pool, so the sanitizers cover what runs on the CPU: this program #includes the library's one
// translation unit (so that it can make a context by hand, without a device, and reach the builders that validate before
// their first HIP call) and is built with -fsanitize=address,undefined for the host side only (tools/asan_host.sh).
// Exercised: spf_ciphertext_{words,from_bincode,to_bincode} (safe_bincode::deserialize of the ciphertext newtypes),
// spf_load_compute_key_bincode's and spf_load_compute_key_nonfft_bincode's size walks (ComputeKey, ComputeKeyNonFft), spf_generate_lut, params_supported / params_generic, and
// spf_graph_add_{input,trivial,op,output} (the reference validates per task, task.rs:26-31) — every call must return a status,
// never crash, never touch memory outside its buffers (every destination is an exact-size heap allocation).  Before the random
// cases, a fixed table calls every spf_*_batch entry point with one bad argument each (batch_forms_refuse_bad_arguments) and
// holds spf_graph_add_op and spf_ciphertext_words to the header's own statement of the ten operations and the four wire
// sizes (graph_ops_match_the_header, wire_sizes_match_the_header).
// Seeds: the reference's own malformed vector (parasol_runtime/src/safe_bincode.rs:58-66, :105-117) and valid serializations.
//
// usage: fuzz_host <cases> [seed]
#include "../spf_amd/csrc/spf_hip.hip"

#include <cinttypes>
#include <random>

namespace {

struct Rng {
    std::mt19937_64 g;
    explicit Rng(uint64_t seed) : g(seed) {}
    uint64_t operator()() { return g(); }
    size_t below(size_t n) { return n ? (size_t)(g() % n) : 0; }
};

std::vector<uint8_t> mutate(const std::vector<uint8_t>& seed, Rng& r)
{
    std::vector<uint8_t> v = seed;
    const int rounds = 1 + (int)r.below(4);
    for (int k = 0; k < rounds; k++) {
        switch (r.below(8)) {
        case 0: if (!v.empty()) v[r.below(v.size())] ^= (uint8_t)(1u << r.below(8)); break;
        case 1: if (!v.empty()) v[r.below(v.size())] = (uint8_t)r(); break;
        case 2: v.resize(r.below(v.size() + 1)); break;                        // truncate
        case 3: v.resize(v.size() + r.below(64), (uint8_t)r()); break;          // trailing bytes
        case 4: {                                                                // a length field of all ones / off by one
            const size_t at = 8 * r.below(v.size() / 8 + 1);
            if (at + 8 <= v.size()) {
                uint64_t n;
                std::memcpy(&n, &v[at], 8);
                const uint64_t choices[6] = {~(uint64_t)0, n + 1, n - 1, 0, (uint64_t)1 << 63, n << 1};
                n = choices[r.below(6)];
                std::memcpy(&v[at], &n, 8);
            }
            break;
        }
        case 5: if (v.size() >= 8) { const uint64_t n = r(); std::memcpy(&v[0], &n, 8); } break; // the first count, random
        case 6: if (!v.empty()) { const size_t a = r.below(v.size()), b = r.below(v.size()); std::swap(v[a], v[b]); } break;
        default: break;
        }
    }
    return v;
}

// a context made by hand: only the fields the host-side validators read (no device: a HIP call that slips through fails at
// hipSetDevice)
void fake_ctx(spf_ctx& c, const spf_params& p, bool generic)
{
    c.prm = p;
    c.device = -1;
    c.generic = generic;
    c.log_n = 0;
    while ((1u << c.log_n) < p.polynomial_degree) c.log_n++;
}

// Every spf_*_batch entry point with exactly one bad argument: each must be refused as SPF_ERR_INVALID_ARGUMENT before its first
// HIP call (the context's device is -1, so a call that reaches HIP returns SPF_ERR_HIP instead).  The buffers are exact-size heap
// allocations for B ciphertexts; the batch-limit cases hand the same buffers with a larger B and must not read them.
bool batch_forms_refuse_bad_arguments(spf_ctx* c)
{
    const spf_params& p = c->prm;
    const size_t B = 2, N = p.polynomial_degree, l = p.cbs_radix_count, nb = 3;
    const size_t l0 = lwe0_words(p), l1 = lwe1_words(p), gw = glwe_words(p), sw = 2 * ggsw_fft_complex(p, p.cbs_radix_count);
    const size_t over_br = (size_t)0x7fffffff + 1, over_tail = (size_t)0x0fffffff + 1; // one past each batch limit
    std::vector<uint64_t> lwe0(B * l0), rhs(B * l0), lwe1(B * l1), glwe(B * gw), glwe_b(B * gw), lut(B * gw), glev(B * l * gw),
        bits(B * nb * gw), o_lwe0(B * l0), o_lwe1(B * l1), o_glwe(B * gw), o_glev(B * l * gw), o_bits(B * nb * l1);
    std::vector<double> ggsw(B * sw), o_ggsw(B * sw), o_ggsw_bits(B * nb * sw);
    bool ok = true;
    auto expect = [&](const char* call, spf_status st) {
        if (st == SPF_ERR_INVALID_ARGUMENT) return;
        fprintf(stderr, "spf_*_batch bad argument: %s returned %d, not SPF_ERR_INVALID_ARGUMENT (%s)\n", call, st, c->err.c_str());
        ok = false;
    };
    expect("keyswitch_lwe_l1_lwe_l0 null in", spf_keyswitch_lwe_l1_lwe_l0_batch(c, B, nullptr, o_lwe0.data()));
    expect("generalized_pbs null lut", spf_generalized_pbs_batch(c, B, lwe0.data(), nullptr, 0, 0, 0, 0, o_glwe.data()));
    expect("generalized_pbs lut_stride 1", spf_generalized_pbs_batch(c, B, lwe0.data(), lut.data(), 1, 0, 0, 0, o_glwe.data()));
    expect("generalized_pbs log_v 12", spf_generalized_pbs_batch(c, B, lwe0.data(), lut.data(), 0, 0, 12, 0, o_glwe.data()));
    expect("generalized_pbs log_chi 52", spf_generalized_pbs_batch(c, B, lwe0.data(), lut.data(), 0, 52, 0, 0, o_glwe.data()));
    expect("generalized_pbs B 0x80000000",
           spf_generalized_pbs_batch(c, over_br, lwe0.data(), lut.data(), 0, 0, 0, 0, o_glwe.data()));
    expect("pbs_univariate lut_stride 1", spf_pbs_univariate_batch(c, B, lwe0.data(), lut.data(), 1, o_lwe1.data()));
    expect("pbs_univariate null in", spf_pbs_univariate_batch(c, B, nullptr, lut.data(), 0, o_lwe1.data()));
    expect("pbs_bivariate null right", spf_pbs_bivariate_batch(c, B, lwe0.data(), nullptr, lut.data(), 0, 2, o_lwe1.data()));
    expect("pbs_bivariate plaintext_bits 64",
           spf_pbs_bivariate_batch(c, B, lwe0.data(), rhs.data(), lut.data(), 0, 64, o_lwe1.data()));
    expect("pbs_bivariate lut_stride 1", spf_pbs_bivariate_batch(c, B, lwe0.data(), rhs.data(), lut.data(), 1, 2, o_lwe1.data()));
    expect("circuit_bootstrap_pbs null out", spf_circuit_bootstrap_pbs_batch(c, B, lwe0.data(), nullptr));
    expect("circuit_bootstrap_pbs B 0x80000000", spf_circuit_bootstrap_pbs_batch(c, over_br, lwe0.data(), o_glwe.data()));
    expect("circuit_bootstrap null in", spf_circuit_bootstrap_batch(c, B, nullptr, o_ggsw.data()));
    expect("circuit_bootstrap B 0x10000000", spf_circuit_bootstrap_batch(c, over_tail, lwe0.data(), o_ggsw.data()));
    expect("mod_switch_trace_and_rotate null out", spf_mod_switch_trace_and_rotate_batch(c, B, glwe.data(), nullptr));
    expect("mod_switch_trace_and_rotate B 0x10000000",
           spf_mod_switch_trace_and_rotate_batch(c, over_tail, glwe.data(), o_glev.data()));
    expect("scheme_switch null in", spf_scheme_switch_batch(c, B, nullptr, o_ggsw.data()));
    expect("scheme_switch B 0x10000000", spf_scheme_switch_batch(c, over_tail, glev.data(), o_ggsw.data()));
    expect("sample_extract_l1 idx N", spf_sample_extract_l1_batch(c, B, glwe.data(), N, o_lwe1.data()));
    expect("sample_extract_l1 null out", spf_sample_extract_l1_batch(c, B, glwe.data(), 0, nullptr));
    expect("glwe_not null in", spf_glwe_not_batch(c, B, nullptr, o_glwe.data()));
    expect("glwe_xor null b", spf_glwe_xor_batch(c, B, glwe.data(), nullptr, o_glwe.data()));
    expect("glwe_mul_xn null out", spf_glwe_mul_xn_batch(c, B, glwe.data(), 3, nullptr));
    expect("glwe_pack n_bits 0", spf_glwe_pack_batch(c, B, 0, bits.data(), o_glwe.data()));
    expect("glwe_pack null out", spf_glwe_pack_batch(c, B, nb, bits.data(), nullptr));
    expect("glwe_unpack_l1 n_bits N + 1", spf_glwe_unpack_l1_batch(c, B, N + 1, glwe.data(), o_bits.data()));
    expect("cmux null sel", spf_cmux_batch(c, B, nullptr, glwe.data(), glwe_b.data(), o_glwe.data()));
    expect("glev_cmux null b", spf_glev_cmux_batch(c, B, ggsw.data(), glev.data(), nullptr, o_glev.data()));
    expect("multiply_glwe_ggsw null ggsw", spf_multiply_glwe_ggsw_batch(c, B, glwe.data(), nullptr, o_glwe.data()));
    expect("gate_bootstrap null in", spf_gate_bootstrap_batch(c, B, nullptr, o_glwe.data()));
    expect("gate_bootstrap B 0x80000000", spf_gate_bootstrap_batch(c, over_br, lwe1.data(), o_glwe.data()));
    expect("keyswitch_circuit_bootstrap null out", spf_keyswitch_circuit_bootstrap_batch(c, B, lwe1.data(), nullptr));
    expect("keyswitch_circuit_bootstrap B 0x10000000",
           spf_keyswitch_circuit_bootstrap_batch(c, over_tail, lwe1.data(), o_ggsw.data()));
    expect("unpack_circuit_bootstrap B * n_bits 0x10000002",
           spf_unpack_circuit_bootstrap_batch(c, over_tail / 2 + 1, 2, glwe.data(), o_ggsw_bits.data()));
    expect("unpack_circuit_bootstrap null in", spf_unpack_circuit_bootstrap_batch(c, B, nb, nullptr, o_ggsw_bits.data()));
    // the standard-form entry points: polynomials and keys as integer words
    std::vector<double> o_spec(B * N);
    expect("poly_fft null in", spf_poly_fft_batch(c, B, nullptr, o_spec.data()));
    expect("poly_fft null out", spf_poly_fft_batch(c, B, glwe.data(), nullptr));
    expect("poly_fft n_polys 0x80000000", spf_poly_fft_batch(c, over_br, glwe.data(), o_spec.data()));
    expect("poly_fft_dev partial overlap", spf_poly_fft_dev(c, nullptr, B, glwe.data(), reinterpret_cast<double*>(glwe.data() + N)));
    expect("load_bootstrap_key_std null", spf_load_bootstrap_key_std(c, nullptr, 2 * (size_t)p.lwe_dimension * ggsw_fft_complex(p, p.pbs_radix_count)));
    expect("load_bootstrap_key_std length in complex", spf_load_bootstrap_key_std(c, glwe.data(), (size_t)p.lwe_dimension * ggsw_fft_complex(p, p.pbs_radix_count)));
    expect("load_automorphism_key_std one word short", spf_load_automorphism_key_std(c, glwe.data(), 2 * ak_complex(p) - 1));
    expect("load_scheme_switch_key_std one word long", spf_load_scheme_switch_key_std(c, glwe.data(), 2 * ssk_complex(p) + 1));
    return ok;
}

// The ten computing `FheOp` arms and the two bootstraps by table as include/spf_hip.h documents them ("Operand order per operation", the gate graphs' comment):
// operation, operand kinds in order, result kind.  Written out here on purpose — NOT read from the library's table (spf_ops.hpp),
// which is what it checks.
struct HeaderOp { spf_graph_op op; int arity; spf_value_kind in[3]; spf_value_kind out; };
const HeaderOp kHeaderOps[12] = {
    {SPF_OP_SAMPLE_EXTRACT, 1, {SPF_VAL_GLWE1}, SPF_VAL_LWE1},
    {SPF_OP_KEYSWITCH_L1_TO_L0, 1, {SPF_VAL_LWE1}, SPF_VAL_LWE0},
    {SPF_OP_CIRCUIT_BOOTSTRAP, 1, {SPF_VAL_LWE0}, SPF_VAL_GGSW1},
    {SPF_OP_SCHEME_SWITCH, 1, {SPF_VAL_GLEV1}, SPF_VAL_GGSW1},
    {SPF_OP_NOT, 1, {SPF_VAL_GLWE1}, SPF_VAL_GLWE1},
    {SPF_OP_GLWE_ADD, 2, {SPF_VAL_GLWE1, SPF_VAL_GLWE1}, SPF_VAL_GLWE1},
    {SPF_OP_MUL_XN, 1, {SPF_VAL_GLWE1}, SPF_VAL_GLWE1},
    {SPF_OP_CMUX, 3, {SPF_VAL_GGSW1, SPF_VAL_GLWE1, SPF_VAL_GLWE1}, SPF_VAL_GLWE1},
    {SPF_OP_GLEV_CMUX, 3, {SPF_VAL_GGSW1, SPF_VAL_GLEV1, SPF_VAL_GLEV1}, SPF_VAL_GLEV1},
    {SPF_OP_MULTIPLY_GGSW_GLWE, 2, {SPF_VAL_GGSW1, SPF_VAL_GLWE1}, SPF_VAL_GLWE1},
    {SPF_OP_PBS_UNIVARIATE, 2, {SPF_VAL_LWE0, SPF_VAL_GLWE1}, SPF_VAL_LWE1},
    {SPF_OP_PBS_BIVARIATE, 3, {SPF_VAL_LWE0, SPF_VAL_LWE0, SPF_VAL_GLWE1}, SPF_VAL_LWE1},
};
const HeaderOp* header_op(int op)
{
    for (const HeaderOp& h : kHeaderOps)
        if (h.op == op) return &h;
    return nullptr;
}

// spf_graph_add_op against kHeaderOps, for every operation: the right operand kinds are accepted and give a node of the stated
// result kind (which spf_graph_add_output takes); a wrong kind in any one slot, one operand too few and one too many are refused
// with the builder's messages; the parameter follows the rule of the header (SampleExtract index below N, MulXN amount mod 2N,
// a bivariate bootstrap's plaintext_bits below 64, ignored elsewhere).  Nothing is run: the context has no device.
bool graph_ops_match_the_header(spf_ctx* c)
{
    const uint64_t N = c->prm.polynomial_degree;
    static uint64_t host_buf[4];
    spf_graph* g = nullptr;
    if (spf_graph_create(c, &g) != SPF_OK) return false;
    bool ok = true;
    auto expect = [&](const char* what, int op, spf_status st, spf_status want, const char* msg) {
        if (st == want && (!msg || c->err == msg)) return;
        fprintf(stderr, "spf_graph_add_op, operation %d, %s: status %d (%s), expected %d (%s)\n", op, what, st, c->err.c_str(), want, msg ? msg : "");
        ok = false;
    };
    uint32_t input_of[5]; // one input node per ciphertext kind
    for (int k = 0; k < 5; k++) expect("input", -1, spf_graph_add_input(g, (spf_value_kind)k, host_buf, &input_of[k]), SPF_OK, nullptr);
    for (const HeaderOp& h : kHeaderOps) {
        uint32_t in[4] = {0, 0, 0, 0}, node = 0;
        for (int s = 0; s < h.arity; s++) in[s] = input_of[h.in[s]];
        in[h.arity] = input_of[h.in[0]];
        expect("right kinds", h.op, spf_graph_add_op(g, h.op, in, h.arity, 0, &node), SPF_OK, nullptr);
        if (ok && (node + 1 != g->nodes.size() || g->nodes[node].kind != h.out || g->nodes[node].n_in != (uint32_t)h.arity)) {
            fprintf(stderr, "spf_graph_add_op, operation %d: the node has kind %d, the header says %d\n", h.op, g->nodes[node].kind, h.out);
            ok = false;
        }
        expect("its node as an output", h.op, spf_graph_add_output(g, node, host_buf), SPF_OK, nullptr);
        const size_t n_nodes = g->nodes.size();
        for (int s = 0; s < h.arity; s++)
            for (int wrong = 0; wrong < 5; wrong++) {
                if (wrong == h.in[s]) continue;
                uint32_t bad[3] = {in[0], in[1], in[2]};
                bad[s] = input_of[wrong];
                expect("a wrong kind in one slot", h.op, spf_graph_add_op(g, h.op, bad, h.arity, 0, &node), SPF_ERR_INVALID_ARGUMENT,
                       "graph op: operand has the wrong ciphertext type");
            }
        expect("one operand too few", h.op, spf_graph_add_op(g, h.op, in, h.arity - 1, 0, &node), SPF_ERR_INVALID_ARGUMENT,
               "graph op: wrong number of operands");
        expect("one operand too many", h.op, spf_graph_add_op(g, h.op, in, h.arity + 1, 0, &node), SPF_ERR_INVALID_ARGUMENT,
               "graph op: wrong number of operands");
        if (h.op == SPF_OP_SAMPLE_EXTRACT)
            expect("index N", h.op, spf_graph_add_op(g, h.op, in, h.arity, N, &node), SPF_ERR_INVALID_ARGUMENT,
                   "graph op: sample_extract index >= polynomial_degree");
        if (h.op == SPF_OP_PBS_BIVARIATE)
            expect("plaintext_bits 64", h.op, spf_graph_add_op(g, h.op, in, h.arity, 64, &node), SPF_ERR_INVALID_ARGUMENT,
                   "graph op: plaintext_bits must be below 64");
        if (g->nodes.size() != n_nodes) { fprintf(stderr, "spf_graph_add_op, operation %d: a refused call left a node\n", h.op); ok = false; }
        // the parameter the node keeps
        const uint64_t given = h.op == SPF_OP_SAMPLE_EXTRACT ? N - 1 : (h.op == SPF_OP_PBS_BIVARIATE ? 63 : 2 * N + 3);
        const uint64_t kept = h.op == SPF_OP_SAMPLE_EXTRACT ? N - 1 : (h.op == SPF_OP_MUL_XN ? 3 : (h.op == SPF_OP_PBS_BIVARIATE ? 63 : 0));
        expect("with a parameter", h.op, spf_graph_add_op(g, h.op, in, h.arity, given, &node), SPF_OK, nullptr);
        if (ok && g->nodes[node].param != kept) {
            fprintf(stderr, "spf_graph_add_op, operation %d: parameter %" PRIu64 " kept as %" PRIu64 ", expected %" PRIu64 "\n", h.op, given, g->nodes[node].param, kept);
            ok = false;
        }
    }
    uint32_t node = 0;
    expect("no such operation", 12, spf_graph_add_op(g, (spf_graph_op)12, &input_of[2], 1, 0, &node), SPF_ERR_INVALID_ARGUMENT, "graph op: unknown operation");
    // the two node constructors of packed integers: n_bits nodes of kind LWE1 with the bit index as parameter / one GLWE1 node
    // whose operand list is kept whole; every refusal of the header, and a refused call leaves nothing behind
    {
        const uint32_t glwe = input_of[SPF_VAL_GLWE1], lwe1 = input_of[SPF_VAL_LWE1];
        std::vector<uint32_t> bits(N + 1, 0), rows(N + 1, glwe);
        const size_t before = g->nodes.size();
        expect("unpack, N bits", -1, spf_graph_add_unpack(g, glwe, N, bits.data()), SPF_OK, nullptr);
        for (uint64_t i = 0; ok && i < N; i++)
            if (bits[i] != before + i || g->nodes[bits[i]].kind != SPF_VAL_LWE1 || g->nodes[bits[i]].param != i || g->nodes[bits[i]].in[0] != glwe) {
                fprintf(stderr, "spf_graph_add_unpack: node %" PRIu64 " is not bit %" PRIu64 " of its operand\n", (uint64_t)bits[i], i);
                ok = false;
            }
        expect("pack, N rows", -1, spf_graph_add_pack(g, rows.data(), N, &node), SPF_OK, nullptr);
        if (ok && (node + 1 != g->nodes.size() || g->nodes[node].kind != SPF_VAL_GLWE1 || g->nodes[node].n_bits != N ||
                   g->pack_in.size() != N || g->nodes[node].ext != 0)) {
            fprintf(stderr, "spf_graph_add_pack: the node does not keep its %" PRIu64 " operands\n", N);
            ok = false;
        }
        expect("the pack node as an output", -1, spf_graph_add_output(g, node, host_buf), SPF_OK, nullptr);
        expect("a bit node as an output", -1, spf_graph_add_output(g, bits[N - 1], host_buf), SPF_OK, nullptr);
        const size_t n_nodes = g->nodes.size();
        const char* range_u = "graph unpack: n_bits must be in 1 ..= polynomial_degree";
        const char* range_p = "graph pack: n_bits must be in 1 ..= polynomial_degree";
        expect("unpack, 0 bits", -1, spf_graph_add_unpack(g, glwe, 0, bits.data()), SPF_ERR_INVALID_ARGUMENT, range_u);
        expect("unpack, N + 1 bits", -1, spf_graph_add_unpack(g, glwe, N + 1, bits.data()), SPF_ERR_INVALID_ARGUMENT, range_u);
        expect("unpack, no such node", -1, spf_graph_add_unpack(g, (uint32_t)n_nodes, 1, bits.data()), SPF_ERR_INVALID_ARGUMENT,
               "graph unpack: operand is not a node of this graph");
        expect("unpack of an LWE", -1, spf_graph_add_unpack(g, lwe1, 1, bits.data()), SPF_ERR_INVALID_ARGUMENT, "graph unpack: operand is not an L1 GLWE");
        expect("unpack, null out", -1, spf_graph_add_unpack(g, glwe, 1, nullptr), SPF_ERR_INVALID_ARGUMENT, "graph unpack: null pointer");
        expect("unpack, null graph", -1, spf_graph_add_unpack(nullptr, glwe, 1, bits.data()), SPF_ERR_INVALID_ARGUMENT, nullptr);
        expect("pack, 0 rows", -1, spf_graph_add_pack(g, rows.data(), 0, &node), SPF_ERR_INVALID_ARGUMENT, range_p);
        expect("pack, N + 1 rows", -1, spf_graph_add_pack(g, rows.data(), N + 1, &node), SPF_ERR_INVALID_ARGUMENT, range_p);
        rows[N - 1] = (uint32_t)n_nodes;
        expect("pack, no such node", -1, spf_graph_add_pack(g, rows.data(), N, &node), SPF_ERR_INVALID_ARGUMENT, "graph pack: operand is not a node of this graph");
        rows[N - 1] = bits[0];
        expect("pack of an LWE", -1, spf_graph_add_pack(g, rows.data(), N, &node), SPF_ERR_INVALID_ARGUMENT, "graph pack: operand is not an L1 GLWE");
        expect("pack, null rows", -1, spf_graph_add_pack(g, nullptr, 1, &node), SPF_ERR_INVALID_ARGUMENT, "graph pack: null pointer");
        expect("pack, null out", -1, spf_graph_add_pack(g, rows.data(), 1, nullptr), SPF_ERR_INVALID_ARGUMENT, "graph pack: null pointer");
        expect("pack, null graph", -1, spf_graph_add_pack(nullptr, rows.data(), 1, &node), SPF_ERR_INVALID_ARGUMENT, nullptr);
        if (g->nodes.size() != n_nodes || g->pack_in.size() != N) { fprintf(stderr, "a refused unpack or pack left a node\n"); ok = false; }
    }
    g->nodes.clear(); // (nothing was planned: no device memory to give back)
    delete g;
    return ok;
}

// spf_ciphertext_words against the formulas in the comments of include/spf_hip.h (spf_value_kind): n+1, k*N+1, (k+1)*N, l_cbs GLWEs;
// the GGSW has no wire format
bool wire_sizes_match_the_header(const spf_params& p)
{
    const size_t n = p.lwe_dimension, k = p.glwe_size, N = p.polynomial_degree, l = p.cbs_radix_count;
    const struct { spf_value_kind kind; size_t words; } want[5] = {
        {SPF_VAL_LWE0, n + 1}, {SPF_VAL_LWE1, k * N + 1}, {SPF_VAL_GLWE1, (k + 1) * N}, {SPF_VAL_GLEV1, l * (k + 1) * N}, {SPF_VAL_GGSW1, 0}};
    bool ok = true;
    for (const auto& w : want)
        if (spf_ciphertext_words(&p, w.kind) != w.words) {
            fprintf(stderr, "spf_ciphertext_words(kind %d) = %zu, the header says %zu\n", w.kind, spf_ciphertext_words(&p, w.kind), w.words);
            ok = false;
        }
    return ok;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc > 1 && !strcmp(argv[1], "--selftest-overflow")) {
        // the sanitizer really watches the library's host code: a caller that lies about `len` makes the parser read past the
        // allocation, and the run must die with a heap-buffer-overflow report (tests/test_asan_host.py expects exactly that)
        spf_params p;
        spf_default_params(&p);
        const size_t w = spf_ciphertext_words(&p, SPF_VAL_LWE0);
        std::unique_ptr<uint8_t[]> bytes(new uint8_t[16]);
        std::memset(bytes.get(), 0, 16);
        const uint64_t n = w;
        std::memcpy(bytes.get(), &n, 8);
        std::unique_ptr<uint64_t[]> out(new uint64_t[w]);
        (void)spf_ciphertext_from_bincode(&p, SPF_VAL_LWE0, bytes.get(), 8 + 8 * w, out.get());
        printf("selftest: no report?!\n");
        return 0;
    }
    const uint64_t cases = argc > 1 ? strtoull(argv[1], nullptr, 10) : 100000;
    Rng r(argc > 2 ? strtoull(argv[2], nullptr, 10) : 0x5EEDF022);
    spf_params dflt;
    spf_default_params(&dflt);
    spf_params tiny = dflt; // a small generic set: the ComputeKey blob stays a few KiB, the walk is the same code
    tiny.lwe_dimension = 2; tiny.polynomial_degree = 16; tiny.ks_radix_count = 2; tiny.tr_radix_count = 2; tiny.ss_radix_count = 2;
    tiny.pbs_radix_log = 4; tiny.cbs_radix_count = 2;

    // seeds
    std::vector<std::vector<uint8_t>> ct_seeds;
    ct_seeds.push_back({253, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0x1, 0x2, 0x3, 0x4}); // the reference's malformed vector
    const spf_value_kind kinds[5] = {SPF_VAL_LWE0, SPF_VAL_LWE1, SPF_VAL_GLWE1, SPF_VAL_GGSW1, SPF_VAL_GLEV1};
    for (const spf_params* p : {&dflt, &tiny})
        for (spf_value_kind k : kinds) {
            const size_t w = spf_ciphertext_words(p, k);
            if (!w) continue;
            std::vector<uint64_t> words(w);
            for (auto& x : words) x = r();
            std::vector<uint8_t> out(8 + 8 * w);
            size_t written = 0;
            if (spf_ciphertext_to_bincode(p, k, words.data(), out.data(), out.size(), &written) == SPF_OK) ct_seeds.push_back(out);
        }
    spf_ctx tiny_ctx, dflt_ctx;
    fake_ctx(tiny_ctx, tiny, true);
    fake_ctx(dflt_ctx, dflt, false);
    if (!batch_forms_refuse_bad_arguments(&dflt_ctx)) return 1;
    if (!graph_ops_match_the_header(&dflt_ctx) || !graph_ops_match_the_header(&tiny_ctx)) return 1;
    if (!wire_sizes_match_the_header(dflt) || !wire_sizes_match_the_header(tiny)) return 1;
    std::vector<uint8_t> key_seed;
    {
        const size_t want[4] = {(size_t)tiny.lwe_dimension * ggsw_fft_complex(tiny, tiny.pbs_radix_count),
                                (size_t)tiny.glwe_size * tiny.polynomial_degree * tiny.ks_radix_count * lwe0_words(tiny), ssk_complex(tiny), ak_complex(tiny)};
        const size_t elem[4] = {16, 8, 16, 16};
        for (int i = 0; i < 4; i++) {
            uint64_t n = want[i];
            for (int b = 0; b < 8; b++) key_seed.push_back((uint8_t)(n >> (8 * b)));
            for (size_t j = 0; j < want[i] * elem[i]; j++) key_seed.push_back((uint8_t)r());
        }
    }
    std::vector<uint8_t> nonfft_seed; // ComputeKeyNonFft: bs_key, ks_key, auto_key, ss_key, every element one u64
    {
        const size_t want[4] = {2 * (size_t)tiny.lwe_dimension * ggsw_fft_complex(tiny, tiny.pbs_radix_count),
                                (size_t)tiny.glwe_size * tiny.polynomial_degree * tiny.ks_radix_count * lwe0_words(tiny), 2 * ak_complex(tiny),
                                2 * ssk_complex(tiny)};
        for (int i = 0; i < 4; i++) {
            uint64_t n = want[i];
            for (int b = 0; b < 8; b++) nonfft_seed.push_back((uint8_t)(n >> (8 * b)));
            for (size_t j = 0; j < want[i] * 8; j++) nonfft_seed.push_back((uint8_t)r());
        }
    }

    uint64_t ok = 0, refused = 0;
    for (uint64_t it = 0; it < cases; it++) {
        const spf_params* p = r.below(2) ? &dflt : &tiny;
        switch (r.below(7)) {
        case 6: { // ComputeKeyNonFft blob: its own size walk; a ComputeKey blob now and then (other field order and element size)
            const std::vector<uint8_t> in = mutate(r.below(4) ? nonfft_seed : key_seed, r);
            std::unique_ptr<uint8_t[]> bytes(new uint8_t[in.size() ? in.size() : 1]);
            if (!in.empty()) std::memcpy(bytes.get(), in.data(), in.size());
            const spf_status st = spf_load_compute_key_nonfft_bincode(&tiny_ctx, bytes.get(), in.size());
            (st == SPF_OK ? ok : refused)++;
            break;
        }
        case 0: case 1: { // ciphertext wire format
            const std::vector<uint8_t> in = mutate(ct_seeds[r.below(ct_seeds.size())], r);
            // an exact-size copy on the heap: a read past `len` is a heap-buffer-overflow under ASan
            std::unique_ptr<uint8_t[]> bytes(new uint8_t[in.size() ? in.size() : 1]);
            if (!in.empty()) std::memcpy(bytes.get(), in.data(), in.size());
            const spf_value_kind k = (spf_value_kind)(r.below(7)); // (5, 6: unknown kinds)
            const size_t w = spf_ciphertext_words(p, k);
            std::unique_ptr<uint64_t[]> out(new uint64_t[w ? w : 1]);
            const spf_status st = spf_ciphertext_from_bincode(p, k, bytes.get(), in.size(), out.get());
            if (st == SPF_OK) {
                ok++;
                std::unique_ptr<uint8_t[]> back(new uint8_t[8 + 8 * w]);
                size_t written = 0;
                const size_t cap = r.below(4) ? 8 + 8 * w : r.below(8 + 8 * w + 1);
                const spf_status st2 = spf_ciphertext_to_bincode(p, k, out.get(), back.get(), cap, &written);
                if ((st2 == SPF_OK) != (cap >= 8 + 8 * w)) { fprintf(stderr, "to_bincode: capacity check is off\n"); return 1; }
                if (st2 == SPF_OK && std::memcmp(back.get(), bytes.get(), 8 + 8 * w) != 0) { fprintf(stderr, "round trip differs\n"); return 1; }
            } else {
                refused++;
            }
            break;
        }
        case 2: { // ComputeKey blob: the size walk (the loaders behind it fail at their first HIP call without a device)
            const std::vector<uint8_t> in = mutate(key_seed, r);
            std::unique_ptr<uint8_t[]> bytes(new uint8_t[in.size() ? in.size() : 1]);
            if (!in.empty()) std::memcpy(bytes.get(), in.data(), in.size());
            const spf_status st = spf_load_compute_key_bincode(&tiny_ctx, bytes.get(), in.size());
            (st == SPF_OK ? ok : refused)++;
            break;
        }
        case 3: { // generate_lut
            const uint32_t bits = (uint32_t)r.below(14);
            const size_t n_maps = r.below(5);
            const size_t n = n_maps << bits;
            std::unique_ptr<uint64_t[]> maps(new uint64_t[n ? n : 1]);
            for (size_t i = 0; i < n; i++) maps[i] = r.below(8) ? r.below((size_t)1 << bits) : r(); // mostly valid values
            const size_t w = (size_t)(p->glwe_size + 1) * p->polynomial_degree;
            std::unique_ptr<uint64_t[]> lut(new uint64_t[w]);
            const spf_status st = spf_generate_lut(p, maps.get(), n_maps, bits, lut.get());
            (st == SPF_OK ? ok : refused)++;
            break;
        }
        case 4: { // parameter validation
            spf_params q = dflt;
            uint32_t* f = reinterpret_cast<uint32_t*>(&q);
            for (int k = 0; k < 3; k++) f[r.below(sizeof(q) / 4)] = r.below(3) ? (uint32_t)r.below(70) : (uint32_t)r();
            std::string why;
            const bool a = params_supported(q, why), b = params_generic(q, why);
            (void)spf_ciphertext_words(&q, (spf_value_kind)r.below(6));
            ((a || b) ? ok : refused)++;
            break;
        }
        default: { // graph builder: random (mostly malformed) node sequences on a hand-made context; nothing is ever run
            spf_graph* g = nullptr;
            if (spf_graph_create(&dflt_ctx, &g) != SPF_OK) { refused++; break; }
            static uint64_t host_buf[4];
            const int n_calls = 1 + (int)r.below(40);
            for (int k = 0; k < n_calls; k++) {
                uint32_t node = 0;
                const uint32_t have = (uint32_t)g->nodes.size();
                spf_status st;
                switch (r.below(4)) {
                case 0: st = spf_graph_add_input(g, (spf_value_kind)r.below(7), r.below(8) ? host_buf : nullptr, &node); break;
                case 1: st = spf_graph_add_trivial(g, (spf_value_kind)r.below(7), r.below(3), &node); break;
                case 2: {
                    uint32_t in[4];
                    for (auto& x : in) x = r.below(4) ? (uint32_t)r.below(have + 2) : (uint32_t)r();
                    st = spf_graph_add_op(g, (spf_graph_op)r.below(14), r.below(10) ? in : nullptr, r.below(5), r.below(2) ? r() : r.below(5000), &node);
                    break;
                }
                default: st = spf_graph_add_output(g, r.below(4) ? (uint32_t)r.below(have + 2) : (uint32_t)r(), r.below(8) ? host_buf : nullptr); break;
                }
                (st == SPF_OK ? ok : refused)++;
            }
            // the builder's invariants: operands precede their users and carry the kind the operation wants
            for (size_t i = 0; i < g->nodes.size(); i++) {
                const auto& n = g->nodes[i];
                if (n.op < 0) continue;
                const HeaderOp* info = header_op(n.op);
                if (!info || n.n_in != (uint32_t)info->arity || n.kind != info->out) { fprintf(stderr, "graph: bad node accepted\n"); return 1; }
                for (uint32_t j = 0; j < n.n_in; j++)
                    if (n.in[j] >= i || g->nodes[n.in[j]].kind != info->in[j]) { fprintf(stderr, "graph: bad operand accepted\n"); return 1; }
            }
            g->nodes.clear(); // (nothing was planned: no device memory to give back)
            delete g;
            break;
        }
        }
    }
    printf("fuzz_host: %" PRIu64 " cases, %" PRIu64 " calls accepted, %" PRIu64 " refused, no sanitizer report\n", cases, ok, refused);
    return 0;
}
