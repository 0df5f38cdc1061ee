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
// cases, a fixed table calls every spf_*_batch entry point with one bad argument each and holds its status and message
// (batch_forms_refuse_bad_arguments), and three more hold spf_graph_add_op, spf_ciphertext_words and the batch shapes to the
// header's own statement of the ten operations, the four wire sizes and every batch entry point's operand widths
// (graph_ops_match_the_header, wire_sizes_match_the_header, batch_shapes_match_the_header).
// Seeds: the reference's own malformed vector (parasol_runtime/src/safe_bincode.rs:58-66, :105-117) and valid serializations.
//
// usage: fuzz_host <cases> [seed]
//        fuzz_host --lifetimes [scenario] | --lifetimes-random <cases> <seed> | --selftest-lifetime   (destroy orders, below)
#include "../spf_amd/csrc/spf_hip.hip"

#include <cinttypes>
#include <functional>
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

// Every spf_*_batch entry point with exactly one bad argument: each must be refused with the stated status AND the stated text of
// spf_last_error before its first HIP call (the context's device is -1, so a call that reaches HIP returns SPF_ERR_HIP instead:
// "reaches the device" below, its text is the runtime's and is not compared).  The buffers are exact-size heap allocations for B
// ciphertexts; the batch-limit cases hand the same buffers with a larger B and must not read them.  The newer forms (blind rotation,
// the functional keyswitches, circuit bootstrap via PFKS, the linear maps) run on a second hand-made context whose readiness flags
// and key shapes are set by hand, each in its `_batch` and its device-pointer form, with null pointers at B == 0, a batch one past
// the limit and an output that overlaps the input; the group forms are held to the checks they make before the batch is split.
// The expected values were recorded from the library as it was before the batch shapes were stated once (spf_ops.hpp).
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
    const spf_status BAD = SPF_ERR_INVALID_ARGUMENT;
    const char* const null_arg = "null argument";
    const char* const too_large = "batch too large";
    const char* const device = nullptr; // SPF_ERR_HIP: every check passed and the call went on to the device
    spf_ctx* on = c;
    // (`msg` null: the text is not compared)
    auto expect = [&](const char* call, spf_status st, spf_status want, const char* msg) {
        if (st != want || (msg && on->err != msg)) {
            fprintf(stderr, "spf_*_batch bad argument: %s returned %d (%s), not %d (%s)\n", call, st, on->err.c_str(), want, msg ? msg : "any text");
            ok = false;
        }
        on->err.clear();
    };
    expect("keyswitch_lwe_l1_lwe_l0 null in", spf_keyswitch_lwe_l1_lwe_l0_batch(c, B, nullptr, o_lwe0.data()), BAD, null_arg);
    expect("generalized_pbs null lut", spf_generalized_pbs_batch(c, B, lwe0.data(), nullptr, 0, 0, 0, 0, o_glwe.data()), BAD, "null lut");
    expect("generalized_pbs lut_stride 1", spf_generalized_pbs_batch(c, B, lwe0.data(), lut.data(), 1, 0, 0, 0, o_glwe.data()), BAD,
           "lut_stride smaller than a GLWE");
    expect("generalized_pbs log_v 12", spf_generalized_pbs_batch(c, B, lwe0.data(), lut.data(), 0, 0, 12, 0, o_glwe.data()), BAD,
           "log_v / log_chi out of range");
    expect("generalized_pbs log_chi 52", spf_generalized_pbs_batch(c, B, lwe0.data(), lut.data(), 0, 52, 0, 0, o_glwe.data()), BAD,
           "log_v / log_chi out of range");
    expect("generalized_pbs B 0x80000000",
           spf_generalized_pbs_batch(c, over_br, lwe0.data(), lut.data(), 0, 0, 0, 0, o_glwe.data()), BAD, too_large);
    expect("pbs_univariate lut_stride 1", spf_pbs_univariate_batch(c, B, lwe0.data(), lut.data(), 1, o_lwe1.data()), BAD,
           "lut_stride smaller than a GLWE");
    expect("pbs_univariate null in", spf_pbs_univariate_batch(c, B, nullptr, lut.data(), 0, o_lwe1.data()), BAD, null_arg);
    expect("pbs_bivariate null right", spf_pbs_bivariate_batch(c, B, lwe0.data(), nullptr, lut.data(), 0, 2, o_lwe1.data()), BAD, null_arg);
    expect("pbs_bivariate plaintext_bits 64",
           spf_pbs_bivariate_batch(c, B, lwe0.data(), rhs.data(), lut.data(), 0, 64, o_lwe1.data()), BAD, "plaintext_bits must be below 64");
    expect("pbs_bivariate lut_stride 1", spf_pbs_bivariate_batch(c, B, lwe0.data(), rhs.data(), lut.data(), 1, 2, o_lwe1.data()), BAD,
           "lut_stride smaller than a GLWE");
    expect("circuit_bootstrap_pbs null out", spf_circuit_bootstrap_pbs_batch(c, B, lwe0.data(), nullptr), BAD, null_arg);
    expect("circuit_bootstrap_pbs B 0x80000000", spf_circuit_bootstrap_pbs_batch(c, over_br, lwe0.data(), o_glwe.data()), BAD, too_large);
    expect("circuit_bootstrap null in", spf_circuit_bootstrap_batch(c, B, nullptr, o_ggsw.data()), BAD, null_arg);
    expect("circuit_bootstrap B 0x10000000", spf_circuit_bootstrap_batch(c, over_tail, lwe0.data(), o_ggsw.data()), BAD, too_large);
    expect("mod_switch_trace_and_rotate null out", spf_mod_switch_trace_and_rotate_batch(c, B, glwe.data(), nullptr), BAD, null_arg);
    expect("mod_switch_trace_and_rotate B 0x10000000",
           spf_mod_switch_trace_and_rotate_batch(c, over_tail, glwe.data(), o_glev.data()), BAD, too_large);
    expect("scheme_switch null in", spf_scheme_switch_batch(c, B, nullptr, o_ggsw.data()), BAD, null_arg);
    expect("scheme_switch B 0x10000000", spf_scheme_switch_batch(c, over_tail, glev.data(), o_ggsw.data()), BAD, too_large);
    expect("sample_extract_l1 idx N", spf_sample_extract_l1_batch(c, B, glwe.data(), N, o_lwe1.data()), BAD,
           "sample_extract index >= polynomial_degree");
    expect("sample_extract_l1 null out", spf_sample_extract_l1_batch(c, B, glwe.data(), 0, nullptr), BAD, null_arg);
    expect("glwe_not null in", spf_glwe_not_batch(c, B, nullptr, o_glwe.data()), BAD, null_arg);
    expect("glwe_xor null b", spf_glwe_xor_batch(c, B, glwe.data(), nullptr, o_glwe.data()), BAD, null_arg);
    expect("glwe_mul_xn null out", spf_glwe_mul_xn_batch(c, B, glwe.data(), 3, nullptr), BAD, null_arg);
    const char* const n_bits_range = "n_bits must be in 1 ..= polynomial_degree";
    const char* const rows_above = "B * n_bits above 0x0fffffff";
    expect("glwe_pack n_bits 0", spf_glwe_pack_batch(c, B, 0, bits.data(), o_glwe.data()), BAD, n_bits_range);
    expect("glwe_pack null out", spf_glwe_pack_batch(c, B, nb, bits.data(), nullptr), BAD, null_arg);
    expect("glwe_unpack_l1 n_bits N + 1", spf_glwe_unpack_l1_batch(c, B, N + 1, glwe.data(), o_bits.data()), BAD, n_bits_range);
    expect("cmux null sel", spf_cmux_batch(c, B, nullptr, glwe.data(), glwe_b.data(), o_glwe.data()), BAD, null_arg);
    expect("glev_cmux null b", spf_glev_cmux_batch(c, B, ggsw.data(), glev.data(), nullptr, o_glev.data()), BAD, null_arg);
    expect("multiply_glwe_ggsw null ggsw", spf_multiply_glwe_ggsw_batch(c, B, glwe.data(), nullptr, o_glwe.data()), BAD, null_arg);
    expect("gate_bootstrap null in", spf_gate_bootstrap_batch(c, B, nullptr, o_glwe.data()), BAD, null_arg);
    expect("gate_bootstrap B 0x80000000", spf_gate_bootstrap_batch(c, over_br, lwe1.data(), o_glwe.data()), BAD, too_large);
    expect("keyswitch_circuit_bootstrap null out", spf_keyswitch_circuit_bootstrap_batch(c, B, lwe1.data(), nullptr), BAD, null_arg);
    expect("keyswitch_circuit_bootstrap B 0x10000000",
           spf_keyswitch_circuit_bootstrap_batch(c, over_tail, lwe1.data(), o_ggsw.data()), BAD, too_large);
    expect("unpack_circuit_bootstrap B * n_bits 0x10000002",
           spf_unpack_circuit_bootstrap_batch(c, over_tail / 2 + 1, 2, glwe.data(), o_ggsw_bits.data()), BAD, rows_above);
    expect("unpack_circuit_bootstrap null in", spf_unpack_circuit_bootstrap_batch(c, B, nb, nullptr, o_ggsw_bits.data()), BAD, null_arg);
    // the standard-form entry points: polynomials and keys as integer words
    std::vector<double> o_spec(B * N);
    expect("poly_fft null in", spf_poly_fft_batch(c, B, nullptr, o_spec.data()), BAD, null_arg);
    expect("poly_fft null out", spf_poly_fft_batch(c, B, glwe.data(), nullptr), BAD, null_arg);
    expect("poly_fft n_polys 0x80000000", spf_poly_fft_batch(c, over_br, glwe.data(), o_spec.data()), BAD, too_large);
    expect("poly_fft_dev partial overlap", spf_poly_fft_dev(c, nullptr, B, glwe.data(), reinterpret_cast<double*>(glwe.data() + N)), BAD,
           "spf_poly_fft_dev: d_out must be d_in itself or must not overlap it");
    const size_t bsk_complex = (size_t)p.lwe_dimension * ggsw_fft_complex(p, p.pbs_radix_count);
    auto key_length = [](const char* name, size_t got, size_t want_complex) {
        return std::string(name) + " key length " + std::to_string(got) + " words != " + std::to_string(2 * want_complex);
    };
    expect("load_bootstrap_key_std null", spf_load_bootstrap_key_std(c, nullptr, 2 * bsk_complex), BAD, null_arg);
    expect("load_bootstrap_key_std length in complex", spf_load_bootstrap_key_std(c, glwe.data(), bsk_complex), BAD,
           key_length("bootstrap", bsk_complex, bsk_complex).c_str());
    expect("load_automorphism_key_std one word short", spf_load_automorphism_key_std(c, glwe.data(), 2 * ak_complex(p) - 1), BAD,
           key_length("automorphism", 2 * ak_complex(p) - 1, ak_complex(p)).c_str());
    expect("load_scheme_switch_key_std one word long", spf_load_scheme_switch_key_std(c, glwe.data(), 2 * ssk_complex(p) + 1), BAD,
           key_length("scheme-switch", 2 * ssk_complex(p) + 1, ssk_complex(p)).c_str());

    // ---- a representative older operation in both forms: nulls at B == 0 are accepted, the limit, the overlap (device-pointer form only)
    expect("cmux nulls at B 0", spf_cmux_batch(c, 0, nullptr, nullptr, nullptr, nullptr), SPF_OK, "");
    expect("glwe_pack nulls at B 0", spf_glwe_pack_batch(c, 0, nb, nullptr, nullptr), SPF_OK, "");
    expect("glwe_pack_dev nulls at B 0", spf_glwe_pack_dev(c, nullptr, 0, nb, nullptr, nullptr), SPF_OK, "");
    expect("glwe_pack B * n_bits one past", spf_glwe_pack_batch(c, 0x0fffffff / nb + 1, nb, bits.data(), o_glwe.data()), BAD, rows_above);
    expect("glwe_pack_dev B * n_bits one past", spf_glwe_pack_dev(c, nullptr, 0x0fffffff / nb + 1, nb, bits.data(), o_glwe.data()), BAD, rows_above);
    expect("glwe_pack_dev out inside in", spf_glwe_pack_dev(c, nullptr, B, nb, bits.data(), bits.data() + gw), BAD,
           "the packed output overlaps the bit GLWEs");
    expect("glwe_pack out inside in reaches the device", spf_glwe_pack_batch(c, B, nb, bits.data(), bits.data() + gw), SPF_ERR_HIP, device);

    // ---- the newer forms, on a context with keys and weights "loaded" by hand
    const size_t k = p.glwe_size, pu_n = 8, pu_p = 2, lin_M = 2, lin_K = 3;
    spf_ctx keyed;
    fake_ctx(keyed, p, c->generic);
    keyed.bsk_ready = true;
    keyed.pufks_ready = true; keyed.pufks_n = (uint32_t)pu_n; keyed.pufks_log = 4; keyed.pufks_count = 4;
    keyed.pfks_ready = true; keyed.pfks_keys = (uint32_t)k + 1; keyed.pfks_n = (uint32_t)(k * N); keyed.pfks_p = 1; keyed.pfks_log = 4; keyed.pfks_count = 4;
    keyed.lin[0].ready = true; keyed.lin[0].M = lin_M; keyed.lin[0].K = lin_K;
    spf_ctx* q = &keyed;
    on = q;
    const size_t ggsw_int = (k + 1) * l * gw; // an integer-form GGSW: as many words as its spectrum
    std::vector<uint64_t> pu_rows(B * pu_p * (pu_n + 1) + B * gw), pf_rows(B * l * l1 + B * ggsw_int), lin_rows(B * (lin_K + lin_M) * l0),
        lwe0_ggsw(B * l0 + B * ggsw_int), rot(B * gw);
    const char* const overlap = "the output overlaps the input";

    expect("blind_rotation nulls at B 0", spf_blind_rotation_batch(q, 0, nb, 0, nullptr, nullptr, nullptr), SPF_OK, "");
    expect("blind_rotation_dev nulls at B 0", spf_blind_rotation_dev(q, nullptr, 0, nb, 0, nullptr, nullptr, nullptr), SPF_OK, "");
    expect("blind_rotation null shift", spf_blind_rotation_batch(q, B, nb, 0, nullptr, glwe.data(), o_glwe.data()), BAD, null_arg);
    expect("blind_rotation n_bits 0", spf_blind_rotation_batch(q, B, 0, 0, ggsw.data(), glwe.data(), o_glwe.data()), BAD, "n_bits must be at least 1");
    expect("blind_rotation n_bits + log_stride 12", spf_blind_rotation_batch(q, B, nb, 9, ggsw.data(), glwe.data(), o_glwe.data()), BAD,
           "n_bits + log_stride above log2(polynomial_degree)");
    expect("blind_rotation B * n_bits one past", spf_blind_rotation_batch(q, 0x0fffffff / nb + 1, nb, 0, ggsw.data(), glwe.data(), o_glwe.data()), BAD, rows_above);
    expect("blind_rotation_dev B * n_bits one past", spf_blind_rotation_dev(q, nullptr, 0x0fffffff / nb + 1, nb, 0, ggsw.data(), glwe.data(), o_glwe.data()), BAD,
           rows_above);
    expect("blind_rotation_dev out == in", spf_blind_rotation_dev(q, nullptr, 1, nb, 0, o_ggsw_bits.data(), rot.data(), rot.data()), BAD,
           "the output overlaps an input");
    expect("blind_rotation_dev out inside shift",
           spf_blind_rotation_dev(q, nullptr, 1, nb, 0, o_ggsw_bits.data(), rot.data(), reinterpret_cast<uint64_t*>(o_ggsw_bits.data() + (nb - 1) * sw)), BAD,
           "the output overlaps an input");
    expect("blind_rotation out == in reaches the device", spf_blind_rotation_batch(q, 1, nb, 0, o_ggsw_bits.data(), rot.data(), rot.data()), SPF_ERR_HIP, device);

    uint64_t* const pu_out = pu_rows.data() + B * pu_p * (pu_n + 1);
    const char* const pu_above = "B * lwe_count above 0x0fffffff";
    expect("public_functional_keyswitch nulls at B 0", spf_public_functional_keyswitch_batch(q, 0, pu_p, nullptr, nullptr), BAD, null_arg);
    expect("public_functional_keyswitch_enqueue nulls at B 0", spf_public_functional_keyswitch_enqueue(q, nullptr, 0, pu_p, nullptr, nullptr), BAD, null_arg);
    expect("public_functional_keyswitch B 0", spf_public_functional_keyswitch_batch(q, 0, pu_p, pu_rows.data(), pu_out), SPF_OK, "");
    expect("public_functional_keyswitch_enqueue B 0", spf_public_functional_keyswitch_enqueue(q, nullptr, 0, pu_p, pu_rows.data(), pu_out), SPF_OK, "");
    expect("public_functional_keyswitch lwe_count 0", spf_public_functional_keyswitch_batch(q, B, 0, pu_rows.data(), pu_out), BAD, "lwe_count must be at least 1");
    expect("public_functional_keyswitch_enqueue lwe_count N + 1", spf_public_functional_keyswitch_enqueue(q, nullptr, B, N + 1, pu_rows.data(), pu_out), BAD,
           "lwe_count above polynomial_degree");
    expect("public_functional_keyswitch B * lwe_count one past", spf_public_functional_keyswitch_batch(q, 0x0fffffff / pu_p + 1, pu_p, pu_rows.data(), pu_out), BAD, pu_above);
    expect("public_functional_keyswitch_enqueue B * lwe_count one past",
           spf_public_functional_keyswitch_enqueue(q, nullptr, 0x0fffffff / pu_p + 1, pu_p, pu_rows.data(), pu_out), BAD, pu_above);
    expect("public_functional_keyswitch_enqueue out on the last input word",
           spf_public_functional_keyswitch_enqueue(q, nullptr, B, pu_p, pu_rows.data(), pu_out - 1), BAD, overlap);
    expect("public_functional_keyswitch_enqueue in on the last output word",
           spf_public_functional_keyswitch_enqueue(q, nullptr, B, pu_p, pu_out + B * gw - 1, pu_out), BAD, overlap);
    expect("public_functional_keyswitch_enqueue out behind in reaches the device",
           spf_public_functional_keyswitch_enqueue(q, nullptr, B, pu_p, pu_rows.data(), pu_out), SPF_ERR_HIP, device);
    expect("public_functional_keyswitch out on the last input word reaches the device",
           spf_public_functional_keyswitch_batch(q, B, pu_p, pu_rows.data(), pu_out - 1), SPF_ERR_HIP, device);
    q->pufks_ready = false;
    expect("public_functional_keyswitch no key", spf_public_functional_keyswitch_batch(q, B, pu_p, pu_rows.data(), pu_out), SPF_ERR_NO_KEY,
           "public functional keyswitch key not loaded");
    expect("public_functional_keyswitch_enqueue no key", spf_public_functional_keyswitch_enqueue(q, nullptr, 0, pu_p, pu_rows.data(), pu_out), SPF_ERR_NO_KEY,
           "public functional keyswitch key not loaded");
    expect("public_functional_keyswitch no key, lwe_count 0", spf_public_functional_keyswitch_batch(q, B, 0, pu_rows.data(), pu_out), BAD, "lwe_count must be at least 1");
    q->pufks_ready = true;

    uint64_t* const pf_out = pf_rows.data() + B * l * l1; // behind B * l rows: room for B GLWEs and for B integer GGSWs
    const char* const pf_none = "private functional keyswitch keys not loaded";
    expect("private_functional_keyswitch nulls at B 0", spf_private_functional_keyswitch_batch(q, 0, 0, nullptr, nullptr), BAD, null_arg);
    expect("private_functional_keyswitch_enqueue nulls at B 0", spf_private_functional_keyswitch_enqueue(q, nullptr, 0, 0, nullptr, nullptr), BAD, null_arg);
    expect("private_functional_keyswitch B 0", spf_private_functional_keyswitch_batch(q, k, 0, pf_rows.data(), pf_out), SPF_OK, "");
    expect("private_functional_keyswitch key_index k + 1", spf_private_functional_keyswitch_batch(q, k + 1, over_tail, pf_rows.data(), pf_out), BAD, "key_index >= n_keys");
    expect("private_functional_keyswitch_enqueue key_index k + 1", spf_private_functional_keyswitch_enqueue(q, nullptr, k + 1, B, pf_rows.data(), pf_out), BAD,
           "key_index >= n_keys");
    expect("private_functional_keyswitch B 0x10000000", spf_private_functional_keyswitch_batch(q, 0, over_tail, pf_rows.data(), pf_out), BAD, too_large);
    expect("private_functional_keyswitch_enqueue B 0x10000000", spf_private_functional_keyswitch_enqueue(q, nullptr, 0, over_tail, pf_rows.data(), pf_out), BAD, too_large);
    expect("private_functional_keyswitch_enqueue out on the last input word",
           spf_private_functional_keyswitch_enqueue(q, nullptr, 0, B, pf_rows.data(), pf_rows.data() + B * l1 - 1), BAD, overlap);
    expect("private_functional_keyswitch_enqueue out behind in reaches the device",
           spf_private_functional_keyswitch_enqueue(q, nullptr, 0, B, pf_rows.data(), pf_rows.data() + B * l1), SPF_ERR_HIP, device);
    expect("private_functional_keyswitch out on the last input word reaches the device",
           spf_private_functional_keyswitch_batch(q, 0, B, pf_rows.data(), pf_rows.data() + B * l1 - 1), SPF_ERR_HIP, device);

    const char* const components = "the GGSW components need n_keys = k+1, lwe_count = 1 and from_dimension = k * N";
    expect("apply_pfks_on_ggsw_components nulls at B 0", spf_apply_pfks_on_ggsw_components_batch(q, 0, nullptr, nullptr), BAD, null_arg);
    expect("apply_pfks_on_ggsw_components_enqueue nulls at B 0", spf_apply_pfks_on_ggsw_components_enqueue(q, nullptr, 0, nullptr, nullptr), BAD, null_arg);
    expect("apply_pfks_on_ggsw_components B 0", spf_apply_pfks_on_ggsw_components_batch(q, 0, pf_rows.data(), pf_out), SPF_OK, "");
    expect("apply_pfks_on_ggsw_components B * l one past", spf_apply_pfks_on_ggsw_components_batch(q, 0x0fffffff / l + 1, pf_rows.data(), pf_out), BAD, too_large);
    expect("apply_pfks_on_ggsw_components_enqueue B * l one past",
           spf_apply_pfks_on_ggsw_components_enqueue(q, nullptr, 0x0fffffff / l + 1, pf_rows.data(), pf_out), BAD, too_large);
    expect("apply_pfks_on_ggsw_components_enqueue out on the last input word",
           spf_apply_pfks_on_ggsw_components_enqueue(q, nullptr, B, pf_rows.data(), pf_out - 1), BAD, overlap);
    expect("apply_pfks_on_ggsw_components_enqueue in on the last output word",
           spf_apply_pfks_on_ggsw_components_enqueue(q, nullptr, 1, pf_out + ggsw_int - 1, pf_out), BAD, overlap);
    expect("apply_pfks_on_ggsw_components_enqueue out behind in reaches the device",
           spf_apply_pfks_on_ggsw_components_enqueue(q, nullptr, B, pf_rows.data(), pf_out), SPF_ERR_HIP, device);
    expect("apply_pfks_on_ggsw_components out on the last input word reaches the device",
           spf_apply_pfks_on_ggsw_components_batch(q, B, pf_rows.data(), pf_out - 1), SPF_ERR_HIP, device);

    uint64_t* const cb_out = lwe0_ggsw.data() + B * l0;
    expect("circuit_bootstrap_via_pfks nulls at B 0", spf_circuit_bootstrap_via_pfks_batch(q, 0, nullptr, nullptr), BAD, null_arg);
    expect("circuit_bootstrap_via_pfks_enqueue nulls at B 0", spf_circuit_bootstrap_via_pfks_enqueue(q, nullptr, 0, nullptr, nullptr), BAD, null_arg);
    expect("circuit_bootstrap_via_pfks B 0", spf_circuit_bootstrap_via_pfks_batch(q, 0, lwe0_ggsw.data(), reinterpret_cast<double*>(cb_out)), SPF_OK, "");
    expect("circuit_bootstrap_via_pfks B * l one past",
           spf_circuit_bootstrap_via_pfks_batch(q, 0x0fffffff / l + 1, lwe0_ggsw.data(), reinterpret_cast<double*>(cb_out)), BAD, too_large);
    expect("circuit_bootstrap_via_pfks_enqueue B * l one past",
           spf_circuit_bootstrap_via_pfks_enqueue(q, nullptr, 0x0fffffff / l + 1, lwe0_ggsw.data(), reinterpret_cast<double*>(cb_out)), BAD, too_large);
    expect("circuit_bootstrap_via_pfks_enqueue out on the last input word",
           spf_circuit_bootstrap_via_pfks_enqueue(q, nullptr, B, lwe0_ggsw.data(), reinterpret_cast<double*>(cb_out - 1)), BAD, overlap);
    expect("circuit_bootstrap_via_pfks_enqueue out behind in reaches the device",
           spf_circuit_bootstrap_via_pfks_enqueue(q, nullptr, B, lwe0_ggsw.data(), reinterpret_cast<double*>(cb_out)), SPF_ERR_HIP, device);
    expect("circuit_bootstrap_via_pfks out on the last input word reaches the device",
           spf_circuit_bootstrap_via_pfks_batch(q, B, lwe0_ggsw.data(), reinterpret_cast<double*>(cb_out - 1)), SPF_ERR_HIP, device);
    q->bsk_ready = false;
    expect("circuit_bootstrap_via_pfks_enqueue no bootstrap key",
           spf_circuit_bootstrap_via_pfks_enqueue(q, nullptr, B, lwe0_ggsw.data(), reinterpret_cast<double*>(cb_out)), SPF_ERR_NO_KEY, "bootstrap key not loaded");
    q->bsk_ready = true;
    q->pfks_p = 2; // keys of another shape: the single operation takes them, the GGSW components do not
    expect("private_functional_keyswitch lwe_count 2: out on the last input word",
           spf_private_functional_keyswitch_enqueue(q, nullptr, 0, 1, pf_rows.data(), pf_rows.data() + 2 * l1 - 1), BAD, overlap);
    expect("apply_pfks_on_ggsw_components lwe_count 2", spf_apply_pfks_on_ggsw_components_batch(q, B, pf_rows.data(), pf_out), BAD, components);
    expect("apply_pfks_on_ggsw_components_enqueue lwe_count 2", spf_apply_pfks_on_ggsw_components_enqueue(q, nullptr, B, pf_rows.data(), pf_out), BAD, components);
    expect("circuit_bootstrap_via_pfks lwe_count 2", spf_circuit_bootstrap_via_pfks_batch(q, B, lwe0_ggsw.data(), reinterpret_cast<double*>(cb_out)), BAD, components);
    expect("circuit_bootstrap_via_pfks_enqueue lwe_count 2",
           spf_circuit_bootstrap_via_pfks_enqueue(q, nullptr, B, lwe0_ggsw.data(), reinterpret_cast<double*>(cb_out)), BAD, components);
    q->pfks_p = 1;
    q->pfks_ready = false;
    expect("private_functional_keyswitch no keys", spf_private_functional_keyswitch_batch(q, k + 1, over_tail, pf_rows.data(), pf_out), SPF_ERR_NO_KEY, pf_none);
    expect("private_functional_keyswitch_enqueue no keys", spf_private_functional_keyswitch_enqueue(q, nullptr, 0, B, pf_rows.data(), pf_out), SPF_ERR_NO_KEY, pf_none);
    expect("apply_pfks_on_ggsw_components no keys", spf_apply_pfks_on_ggsw_components_batch(q, B, pf_rows.data(), pf_out), SPF_ERR_NO_KEY, pf_none);
    expect("circuit_bootstrap_via_pfks_enqueue no keys",
           spf_circuit_bootstrap_via_pfks_enqueue(q, nullptr, B, lwe0_ggsw.data(), reinterpret_cast<double*>(cb_out)), SPF_ERR_NO_KEY, pf_none);
    q->pfks_ready = true;

    uint64_t* const lin_out = lin_rows.data() + B * lin_K * l0;
    expect("lwe_linear nulls at B 0", spf_lwe_linear_batch(q, 0, SPF_VAL_LWE0, 0, nullptr, nullptr), BAD, null_arg);
    expect("lwe_linear_enqueue nulls at B 0", spf_lwe_linear_enqueue(q, nullptr, 0, SPF_VAL_LWE0, 0, nullptr, nullptr), BAD, null_arg);
    expect("lwe_linear B 0", spf_lwe_linear_batch(q, 0, SPF_VAL_LWE0, 0, lin_rows.data(), lin_out), SPF_OK, "");
    expect("lwe_linear_enqueue B 0", spf_lwe_linear_enqueue(q, nullptr, 0, SPF_VAL_LWE1, 0, lin_rows.data(), lin_out), SPF_OK, "");
    expect("lwe_linear slot 64", spf_lwe_linear_batch(q, 64, SPF_VAL_LWE0, B, lin_rows.data(), lin_out), BAD, "slot 64 >= SPF_LWE_LINEAR_SLOTS = 64");
    expect("lwe_linear_enqueue kind GLWE1", spf_lwe_linear_enqueue(q, nullptr, 0, SPF_VAL_GLWE1, B, lin_rows.data(), lin_out), BAD,
           "kind must be SPF_VAL_LWE0 or SPF_VAL_LWE1");
    expect("lwe_linear empty slot", spf_lwe_linear_batch(q, 1, SPF_VAL_LWE0, B, lin_rows.data(), lin_out), SPF_ERR_NO_KEY, "no weights loaded in slot 1");
    expect("lwe_linear B * max(M, K) one past", spf_lwe_linear_batch(q, 0, SPF_VAL_LWE0, 0x0fffffff / lin_K + 1, lin_rows.data(), lin_out), BAD, too_large);
    expect("lwe_linear_enqueue B * max(M, K) one past",
           spf_lwe_linear_enqueue(q, nullptr, 0, SPF_VAL_LWE0, 0x0fffffff / lin_K + 1, lin_rows.data(), lin_out), BAD, too_large);
    expect("lwe_linear out on the last input word", spf_lwe_linear_batch(q, 0, SPF_VAL_LWE0, B, lin_rows.data(), lin_out - 1), BAD, overlap);
    expect("lwe_linear_enqueue out on the last input word", spf_lwe_linear_enqueue(q, nullptr, 0, SPF_VAL_LWE0, B, lin_rows.data(), lin_out - 1), BAD, overlap);
    expect("lwe_linear_enqueue in on the last output word",
           spf_lwe_linear_enqueue(q, nullptr, 0, SPF_VAL_LWE0, 1, lin_out + lin_M * l0 - 1, lin_out), BAD, overlap);
    expect("lwe_linear out behind in reaches the device", spf_lwe_linear_batch(q, 0, SPF_VAL_LWE0, B, lin_rows.data(), lin_out), SPF_ERR_HIP, device);
    expect("lwe_linear_enqueue out behind in reaches the device", spf_lwe_linear_enqueue(q, nullptr, 0, SPF_VAL_LWE0, B, lin_rows.data(), lin_out), SPF_ERR_HIP, device);

    // ---- the group forms, up to the point where the batch would be split: one hand-made member (its thread is never started, so
    // every call here must return before group_split posts a range); the text is spf_group_last_error's
    spf_group* grp = new spf_group();
    grp->prm = p;
    grp->m.emplace_back(new spf_group::Member());
    spf_ctx* m0 = new spf_ctx();
    fake_ctx(*m0, p, c->generic);
    m0->pufks_ready = true; m0->pufks_n = (uint32_t)pu_n; m0->pufks_log = 4; m0->pufks_count = 4;
    m0->pfks_ready = true; m0->pfks_keys = (uint32_t)k + 1; m0->pfks_n = (uint32_t)(k * N); m0->pfks_p = 1; m0->pfks_log = 4; m0->pfks_count = 4;
    m0->lin[0].ready = true; m0->lin[0].M = lin_M; m0->lin[0].K = lin_K;
    grp->m.back()->ctx = m0;
    grp->m.back()->device = -1;
    auto gexpect = [&](const char* call, spf_status st, spf_status want, const char* msg, spf_group* of) {
        const std::string got = spf_group_last_error(of);
        if (st != want || got != msg) {
            fprintf(stderr, "spf_group_*_batch bad argument: %s returned %d (%s), not %d (%s)\n", call, st, got.c_str(), want, msg);
            ok = false;
        }
        gfail(of, SPF_OK, "");
    };
    gexpect("group glwe_not null group", spf_group_glwe_not_batch(nullptr, B, glwe.data(), o_glwe.data()), BAD, "null group", nullptr);
    gexpect("group glwe_not null in", spf_group_glwe_not_batch(grp, B, nullptr, o_glwe.data()), BAD, null_arg, grp);
    gexpect("group glwe_not nulls at B 0", spf_group_glwe_not_batch(grp, 0, nullptr, nullptr), SPF_OK, "", grp);
    gexpect("group cmux null b", spf_group_cmux_batch(grp, B, ggsw.data(), glwe.data(), nullptr, o_glwe.data()), BAD, null_arg, grp);
    gexpect("group pbs_bivariate plaintext_bits 64", spf_group_pbs_bivariate_batch(grp, 0, nullptr, nullptr, nullptr, 0, 64, nullptr), BAD,
            "plaintext_bits must be below 64", grp);
    gexpect("group glwe_pack n_bits 0", spf_group_glwe_pack_batch(grp, 0, 0, nullptr, nullptr), BAD, n_bits_range, grp);
    gexpect("group glwe_unpack_l1 null out", spf_group_glwe_unpack_l1_batch(grp, B, 0, glwe.data(), nullptr), BAD, null_arg, grp);
    gexpect("group unpack_circuit_bootstrap B * n_bits one past",
            spf_group_unpack_circuit_bootstrap_batch(grp, 0x0fffffff / nb + 1, nb, glwe.data(), o_ggsw_bits.data()), BAD, rows_above, grp);
    gexpect("group blind_rotation nulls at B 0", spf_group_blind_rotation_batch(grp, 0, nb, 0, nullptr, nullptr, nullptr), SPF_OK, "", grp);
    gexpect("group blind_rotation n_bits 0", spf_group_blind_rotation_batch(grp, 0, 0, 0, nullptr, nullptr, nullptr), BAD, "n_bits must be at least 1", grp);
    gexpect("group blind_rotation B * n_bits one past",
            spf_group_blind_rotation_batch(grp, 0x0fffffff / nb + 1, nb, 0, ggsw.data(), glwe.data(), o_glwe.data()), BAD, rows_above, grp);
    gexpect("group public_functional_keyswitch null group", spf_group_public_functional_keyswitch_batch(nullptr, 0, pu_p, pu_rows.data(), pu_out), BAD, "null group", nullptr);
    gexpect("group public_functional_keyswitch nulls at B 0", spf_group_public_functional_keyswitch_batch(grp, 0, pu_p, nullptr, nullptr), BAD, null_arg, grp);
    gexpect("group public_functional_keyswitch B 0", spf_group_public_functional_keyswitch_batch(grp, 0, pu_p, pu_rows.data(), pu_out), SPF_OK, "", grp);
    gexpect("group public_functional_keyswitch lwe_count 0", spf_group_public_functional_keyswitch_batch(grp, B, 0, pu_rows.data(), pu_out), BAD,
            "lwe_count must be at least 1", grp);
    gexpect("group public_functional_keyswitch B * lwe_count one past",
            spf_group_public_functional_keyswitch_batch(grp, 0x0fffffff / pu_p + 1, pu_p, pu_rows.data(), pu_out), BAD, pu_above, grp);
    m0->pufks_ready = false;
    gexpect("group public_functional_keyswitch no key", spf_group_public_functional_keyswitch_batch(grp, 0, pu_p, pu_rows.data(), pu_out), SPF_ERR_NO_KEY,
            "public functional keyswitch key not loaded", grp);
    gexpect("group public_functional_keyswitch no key, lwe_count 0", spf_group_public_functional_keyswitch_batch(grp, B, 0, pu_rows.data(), pu_out), BAD,
            "lwe_count must be at least 1", grp);
    gexpect("group private_functional_keyswitch nulls at B 0", spf_group_private_functional_keyswitch_batch(grp, 0, 0, nullptr, nullptr), BAD, null_arg, grp);
    gexpect("group private_functional_keyswitch B 0", spf_group_private_functional_keyswitch_batch(grp, k, 0, pf_rows.data(), pf_out), SPF_OK, "", grp);
    gexpect("group private_functional_keyswitch key_index k + 1", spf_group_private_functional_keyswitch_batch(grp, k + 1, over_tail, pf_rows.data(), pf_out), BAD,
            "key_index >= n_keys", grp);
    gexpect("group private_functional_keyswitch B 0x10000000", spf_group_private_functional_keyswitch_batch(grp, 0, over_tail, pf_rows.data(), pf_out), BAD, too_large, grp);
    m0->pfks_ready = false;
    gexpect("group private_functional_keyswitch no keys", spf_group_private_functional_keyswitch_batch(grp, k + 1, over_tail, pf_rows.data(), pf_out), SPF_ERR_NO_KEY,
            pf_none, grp);
    gexpect("group circuit_bootstrap_via_pfks nulls at B 0, no keys", spf_group_circuit_bootstrap_via_pfks_batch(grp, 0, nullptr, nullptr), SPF_OK, "", grp);
    gexpect("group circuit_bootstrap_via_pfks null out", spf_group_circuit_bootstrap_via_pfks_batch(grp, B, lwe0_ggsw.data(), nullptr), BAD, null_arg, grp);
    gexpect("group lwe_linear nulls at B 0", spf_group_lwe_linear_batch(grp, 0, SPF_VAL_LWE0, 0, nullptr, nullptr), BAD, null_arg, grp);
    gexpect("group lwe_linear B 0", spf_group_lwe_linear_batch(grp, 0, SPF_VAL_LWE0, 0, lin_rows.data(), lin_out), SPF_OK, "", grp);
    gexpect("group lwe_linear slot 64", spf_group_lwe_linear_batch(grp, 64, SPF_VAL_LWE0, B, lin_rows.data(), lin_out), BAD, "slot 64 >= SPF_LWE_LINEAR_SLOTS = 64", grp);
    gexpect("group lwe_linear kind GGSW1", spf_group_lwe_linear_batch(grp, 0, SPF_VAL_GGSW1, B, lin_rows.data(), lin_out), BAD,
            "kind must be SPF_VAL_LWE0 or SPF_VAL_LWE1", grp);
    gexpect("group lwe_linear empty slot", spf_group_lwe_linear_batch(grp, 1, SPF_VAL_LWE0, B, lin_rows.data(), lin_out), SPF_ERR_NO_KEY, "no weights loaded in slot 1", grp);
    gexpect("group lwe_linear B * max(M, K) one past", spf_group_lwe_linear_batch(grp, 0, SPF_VAL_LWE0, 0x0fffffff / lin_K + 1, lin_rows.data(), lin_out), BAD,
            too_large, grp);
    gexpect("group lwe_linear out on the last input word", spf_group_lwe_linear_batch(grp, 0, SPF_VAL_LWE0, B, lin_rows.data(), lin_out - 1), BAD, overlap, grp);
    spf_group_destroy(grp);
    return ok;
}

// The operand and result widths of every spf_*_batch entry point, in 64-bit words per item, as the sentences of include/spf_hip.h
// state them (a complex bin is two words) — written out here on purpose, NOT computed with the library's size helpers — against
// the batch shapes of spf_ops.hpp that the three forms of each entry point share.  Operands in the order the shape lists them
// (the order they are staged in: a selector or spectrum first); `max`: the batch limit where the header states one, else 0.
bool batch_shapes_match_the_header(const spf_params& p)
{
    const size_t n = p.lwe_dimension, k = p.glwe_size, N = p.polynomial_degree, l = p.cbs_radix_count;
    const size_t lwe0 = n + 1, lwe1 = k * N + 1, glwe = (k + 1) * N, glev = l * (k + 1) * N, ggsw = 2 * ((k + 1) * l * (k + 1) * N / 2);
    const size_t n_bits = 3, stride = glwe + 5, lwe_count = 2, from = 9, M = 5, K = 7;
    const int L0 = SPF_VAL_LWE0, L1 = SPF_VAL_LWE1, GL = SPF_VAL_GLWE1, GG = SPF_VAL_GGSW1;
    const struct { const char* entry; BatchShape got; int n_in; size_t in[3]; size_t out; size_t max; } rows[] = {
        {"poly_fft", poly_fft_shape(p), 1, {N}, 2 * (N / 2), 0},
        {"keyswitch_lwe_l1_lwe_l0", spf_ops::shape(p, spf_ops::OP_KEYSWITCH), 1, {lwe1}, lwe0, 0},
        {"generalized_pbs", pbs_shape(p, false, false, stride), 2, {lwe0, stride}, glwe, 0},
                {"pbs_univariate", pbs_shape(p, true, false, stride), 2, {lwe0, stride}, lwe1, 0},
        {"pbs_bivariate", pbs_shape(p, true, true, stride), 3, {lwe0, lwe0, stride}, lwe1, 0},
        {"circuit_bootstrap_pbs", pbs_shape(p, false), 2, {lwe0, 0}, glwe, 0},
        {"circuit_bootstrap", spf_ops::shape(p, spf_ops::OP_CBS), 1, {lwe0}, ggsw, 0},
        {"mod_switch_trace_and_rotate", trace_shape(p), 1, {glwe}, glev, 0},
        {"scheme_switch", spf_ops::shape(p, spf_ops::OP_SCHEME_SWITCH), 1, {glev}, ggsw, 0},
        {"sample_extract_l1", spf_ops::shape(p, spf_ops::OP_SAMPLE_EXTRACT), 1, {glwe}, lwe1, 0},
        {"glwe_not", spf_ops::shape(p, spf_ops::OP_NOT), 1, {glwe}, glwe, 0},
        {"glwe_mul_xn", spf_ops::shape(p, spf_ops::OP_MUL_XN), 1, {glwe}, glwe, 0},
        {"glwe_xor", spf_ops::shape(p, spf_ops::OP_GLWE_ADD), 2, {glwe, glwe}, glwe, 0},
        {"cmux", spf_ops::shape(p, spf_ops::OP_CMUX), 3, {ggsw, glwe, glwe}, glwe, 0},
        {"glev_cmux", spf_ops::shape(p, spf_ops::OP_GLEV_CMUX), 3, {ggsw, glev, glev}, glev, 0},
        {"multiply_glwe_ggsw", spf_ops::shape(p, spf_ops::OP_MULTIPLY_GGSW_GLWE), 2, {ggsw, glwe}, glwe, 0},
        {"gate_bootstrap", gate_bootstrap_shape(p), 1, {lwe1}, glwe, 0},
        {"keyswitch_circuit_bootstrap", spf_ops::shape(p, spf_ops::OP_GATE_CBS), 1, {lwe1}, ggsw, 0},
        {"glwe_pack", packed_shape(p, n_bits, GL, GL, true), 1, {n_bits * glwe}, glwe, 0x0fffffff / n_bits},
        {"glwe_unpack_l1", packed_shape(p, n_bits, GL, L1, false), 1, {glwe}, n_bits * lwe1, 0x0fffffff / n_bits},
        {"unpack_circuit_bootstrap", packed_shape(p, n_bits, GL, GG, false), 1, {glwe}, n_bits * ggsw, 0x0fffffff / n_bits},
        {"blind_rotation", blind_rotation_shape(p, n_bits), 2, {n_bits * ggsw, glwe}, glwe, 0x0fffffff / n_bits},
        {"public_functional_keyswitch", pufks_shape(p, lwe_count, from), 1, {lwe_count * (from + 1)}, glwe, 0x0fffffff / lwe_count},
        {"private_functional_keyswitch", pfks_shape(p, lwe_count * (from + 1)), 1, {lwe_count * (from + 1)}, glwe, 0x0fffffff},
        {"apply_pfks_on_ggsw_components", pfks_components_shape(p, lwe1), 1, {l * lwe1}, (k + 1) * l * (k + 1) * N, 0},
        {"circuit_bootstrap_via_pfks", cbs_via_pfks_shape(p), 1, {lwe0}, ggsw, 0},
        {"lwe_linear, level 0", lwe_linear_batch_shape(p, M, K, L0), 1, {K * lwe0}, M * lwe0, 0},
        {"lwe_linear, level 1", lwe_linear_batch_shape(p, M, K, L1), 1, {K * lwe1}, M * lwe1, 0},
    };
    bool ok = true;
    for (const auto& r : rows) {
        bool same = r.got.n_in == r.n_in && r.got.out_words == r.out && (!r.max || r.got.max_batch == r.max);
        for (int i = 0; i < 3; i++) same = same && r.got.in_words[i] == r.in[i];
        if (same) continue;
        fprintf(stderr, "batch shape of %s: %d operands of %zu / %zu / %zu words, result %zu, limit %zu; the header says %d of %zu / %zu / %zu, result %zu, limit %zu\n",
                r.entry, r.got.n_in, r.got.in_words[0], r.got.in_words[1], r.got.in_words[2], r.got.out_words, r.got.max_batch, r.n_in, r.in[0], r.in[1],
                r.in[2], r.out, r.max);
        ok = false;
    }
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
    // the GLWE keyswitch, automorphism round and trace (SPF_OP_GLWE_* = 12 .. 14): one GLWE1 in, one GLWE1 out, recorded as the
    // nodes of their named constructors (kinds 70 .. 72); the slot below SPF_GLWE_KSK_SLOTS, the round in 1 .. log2 N, the trace's
    // parameter ignored
    {
        uint32_t log_n = 0;
        while (((uint64_t)1 << (log_n + 1)) <= N) log_n++;
        const struct { spf_graph_op op; int32_t kind; uint64_t good, kept, bad; const char* why; } glwe_ops[3] = {
            {SPF_OP_GLWE_KEYSWITCH, 70, SPF_GLWE_KSK_SLOTS - 1, SPF_GLWE_KSK_SLOTS - 1, SPF_GLWE_KSK_SLOTS, "graph op: slot 16 >= SPF_GLWE_KSK_SLOTS = 16"},
            {SPF_OP_GLWE_AUTOMORPHISM, 71, log_n, log_n, 0, nullptr},
            {SPF_OP_GLWE_TRACE, 72, 2 * N + 3, 0, 0, nullptr}};
        for (const auto& h : glwe_ops) {
            const uint32_t in[2] = {input_of[SPF_VAL_GLWE1], input_of[SPF_VAL_GLWE1]};
            expect("right kind", h.op, spf_graph_add_op(g, h.op, in, 1, h.good, &node), SPF_OK, nullptr);
            if (ok && (node + 1 != g->nodes.size() || g->nodes[node].kind != SPF_VAL_GLWE1 || g->nodes[node].op != h.kind || g->nodes[node].param != h.kept)) {
                fprintf(stderr, "spf_graph_add_op, operation %d: not the node of its named constructor\n", h.op);
                ok = false;
            }
            const size_t n_nodes = g->nodes.size();
            for (int wrong = 0; wrong < 5; wrong++)
                if (wrong != SPF_VAL_GLWE1) expect("a wrong kind", h.op, spf_graph_add_op(g, h.op, &input_of[wrong], 1, h.good, &node), SPF_ERR_INVALID_ARGUMENT, nullptr);
            // (over another number of operands the value names no operation of this door: "unknown operation", with value and count)
            expect("no operand", h.op, spf_graph_add_op(g, h.op, in, 0, h.good, &node), SPF_ERR_INVALID_ARGUMENT, nullptr);
            if (c->err.find("graph op: unknown operation: value " + std::to_string((int)h.op) + " over 0 operands") != 0) { fprintf(stderr, "spf_graph_add_op, operation %d, no operand: %s\n", h.op, c->err.c_str()); ok = false; }
            expect("one operand too many", h.op, spf_graph_add_op(g, h.op, in, 2, h.good, &node), SPF_ERR_INVALID_ARGUMENT, nullptr);
            if (c->err.find("graph op: unknown operation: value " + std::to_string((int)h.op) + " over 2 operands") != 0) { fprintf(stderr, "spf_graph_add_op, operation %d, two operands: %s\n", h.op, c->err.c_str()); ok = false; }
            if (h.op != SPF_OP_GLWE_TRACE) expect("a parameter out of range", h.op, spf_graph_add_op(g, h.op, in, 1, h.bad, &node), SPF_ERR_INVALID_ARGUMENT, h.why);
            if (h.op == SPF_OP_GLWE_AUTOMORPHISM) expect("round log2 N + 1", h.op, spf_graph_add_op(g, h.op, in, 1, log_n + 1, &node), SPF_ERR_INVALID_ARGUMENT, nullptr);
            if (g->nodes.size() != n_nodes) { fprintf(stderr, "spf_graph_add_op, operation %d: a refused call left a node\n", h.op); ok = false; }
        }
    }
    expect("no such operation", 15, spf_graph_add_op(g, (spf_graph_op)15, &input_of[2], 1, 0, &node), SPF_ERR_INVALID_ARGUMENT, "graph op: unknown operation");
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
        if (ok && (node + 1 != g->nodes.size() || g->nodes[node].kind != SPF_VAL_GLWE1 || g->nodes[node].count != N ||
                   g->listed_operands() != N || g->nodes[node].list_at != 0)) {
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
        if (g->nodes.size() != n_nodes || g->listed_operands() != N) { fprintf(stderr, "a refused unpack or pack left a node\n"); ok = false; }
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


// ---- lifetimes: every destroy order of the handles (contexts, groups, graphs, jobs), on hand-made parents, no device ----------
//
// The rule of include/spf_hip.h ("Lifetimes"): a child keeps its parent alive, destroy functions may come in any order.  A forest
// of hand-made contexts and groups (as fake_ctx: device -1, every HIP call fails and is ignored by the destroy paths) with graphs,
// jobs, jobs filed under a hand-filled merged entry and graphs on borrowed member contexts is taken apart in a given or a random
// order; after every step spf_live_objects must equal the model below, which knows the rule and nothing of the library's
// counting.  The sanitizers see a parent freed under a child, LeakSanitizer one that nobody freed.
struct Forest {
    enum Type { CTX = 0, GROUP = 1, GRAPH = 2 };
    struct Handle { Type type; int idx; };
    struct MCtx { spf_ctx* h; bool held; int kids; };                       // held: by the caller, or by its group; kids: graphs on it
    struct MSlot { std::vector<int> jobs; bool graph = false; };          // one merged[member] entry: the jobs filed there
    struct MGroup { spf_group* h; bool held; int jobs; std::vector<int> ctx; std::vector<MSlot> slots; bool freed; };
    struct MGraph { spf_graph* h; int ctx; int grp; bool alive; };
    spf_params prm;
    std::vector<MCtx> ctxs;
    std::vector<MGroup> groups;
    std::vector<MGraph> graphs;
    std::vector<Handle> handles; // what the caller owns and has to destroy, in creation order
    uint64_t merged_alive = 0;
    bool ok = true;
    const char* step = "";

    explicit Forest(const spf_params& p) : prm(p) {}

    void check()
    {
        uint64_t want_ctx = 0, want_grp = 0, want_graph = merged_alive;
        for (const MCtx& c : ctxs) want_ctx += (c.held || c.kids > 0) ? 1 : 0;
        for (const MGroup& g : groups) want_grp += g.freed ? 0 : 1;
        for (const MGraph& g : graphs) want_graph += g.alive ? 1 : 0;
        spf_live_counts got;
        if (spf_live_objects(&got) != SPF_OK) { fprintf(stderr, "spf_live_objects failed\n"); ok = false; return; }
        if (got.contexts != want_ctx || got.groups != want_grp || got.graphs != want_graph || got.pools != 0 || got.values != 0) {
            fprintf(stderr, "lifetimes, after %s: live contexts/groups/graphs/pools/values %" PRIu64 "/%" PRIu64 "/%" PRIu64 "/%" PRIu64 "/%" PRIu64
                            ", the model says %" PRIu64 "/%" PRIu64 "/%" PRIu64 "/0/0\n",
                    step, got.contexts, got.groups, got.graphs, got.pools, got.values, want_ctx, want_grp, want_graph);
            ok = false;
        }
    }
    int new_ctx()
    {
        spf_ctx* c = new spf_ctx();
        fake_ctx(*c, prm, true);
        ctxs.push_back({c, true, 0});
        return (int)ctxs.size() - 1;
    }
    int add_ctx()
    {
        const int i = new_ctx();
        handles.push_back({CTX, i});
        step = "a context made";
        check();
        return i;
    }
    int add_group(int members)
    {
        spf_group* g = new spf_group();
        g->prm = prm;
        MGroup m{g, true, 0, {}, {}, false};
        for (int i = 0; i < members; i++) {
            const int c = new_ctx();
            g->m.emplace_back(new spf_group::Member());
            g->m.back()->ctx = ctxs[(size_t)c].h;
            g->m.back()->device = -1;
            m.ctx.push_back(c);
        }
        g->merged.resize((size_t)members);
        m.slots.resize((size_t)members);
        groups.push_back(m);
        handles.push_back({GROUP, (int)groups.size() - 1});
        step = "a group made";
        check();
        return (int)groups.size() - 1;
    }
    // nodes through the builder, so that the graph owns host memory of its own
    void fill(spf_graph* g, size_t n_ops)
    {
        static uint64_t host_buf[4];
        uint32_t at = 0, node = 0;
        if (spf_graph_add_input(g, SPF_VAL_GLWE1, host_buf, &at) != SPF_OK) ok = false;
        for (size_t k = 0; k < n_ops; k++) {
            if (spf_graph_add_op(g, SPF_OP_NOT, &at, 1, 0, &node) != SPF_OK) ok = false;
            at = node;
        }
        if (spf_graph_add_output(g, at, host_buf) != SPF_OK) ok = false;
    }
    // a graph on context `c` (a caller's, or one borrowed from a group: spf_group_ctx)
    int add_graph(int c, size_t n_ops = 2)
    {
        spf_graph* g = nullptr;
        if (spf_graph_create(ctxs[(size_t)c].h, &g) != SPF_OK) { ok = false; return -1; }
        fill(g, n_ops);
        ctxs[(size_t)c].kids++;
        graphs.push_back({g, c, -1, true});
        handles.push_back({GRAPH, (int)graphs.size() - 1});
        step = "a graph made";
        check();
        return (int)graphs.size() - 1;
    }
    int add_borrowed_graph(int grp, int member, size_t n_ops = 2)
    {
        if (spf_group_ctx(groups[(size_t)grp].h, member) != ctxs[(size_t)groups[(size_t)grp].ctx[(size_t)member]].h) ok = false;
        return add_graph(groups[(size_t)grp].ctx[(size_t)member], n_ops);
    }
    // a job of group `grp`; slot >= 0: to be filed under merged[slot] by file_merged()
    int add_job(int grp, int slot = -1, size_t n_ops = 2)
    {
        MGroup& m = groups[(size_t)grp];
        spf_graph* g = nullptr;
        if (spf_group_graph_create(m.h, &g) != SPF_OK) { ok = false; return -1; }
        fill(g, n_ops);
        ctxs[(size_t)m.ctx[0]].kids++; // (a job is built on member 0's context)
        m.jobs++;
        graphs.push_back({g, m.ctx[0], grp, true});
        const int k = (int)graphs.size() - 1;
        if (slot >= 0) m.slots[(size_t)slot].jobs.push_back(k);
        handles.push_back({GRAPH, k});
        step = "a job made";
        check();
        return k;
    }
    // what a run of the group leaves behind, filled in by hand: per member with filed jobs one merged graph on that member's
    // context (spf_graph_create) and the list of its jobs
    void file_merged()
    {
        for (MGroup& m : groups)
            for (size_t s = 0; s < m.slots.size(); s++) {
                if (m.slots[s].jobs.empty()) continue;
                spf_group::Merged& mg = m.h->merged[s];
                if (spf_graph_create(ctxs[(size_t)m.ctx[s]].h, &mg.graph) != SPF_OK) { ok = false; continue; }
                for (int k : m.slots[s].jobs) {
                    mg.jobs.push_back(graphs[(size_t)k].h);
                    mg.shape.emplace_back(graphs[(size_t)k].h->nodes.size(), graphs[(size_t)k].h->outputs.size());
                }
                m.slots[s].graph = true;
                ctxs[(size_t)m.ctx[s]].kids++;
                merged_alive++;
                step = "a merged graph filed";
                check();
            }
    }
    void drop_merged(MGroup& m, size_t s)
    {
        if (!m.slots[s].graph) return;
        m.slots[s].graph = false;
        m.slots[s].jobs.clear();
        ctxs[(size_t)m.ctx[s]].kids--;
        merged_alive--;
    }
    void maybe_free(MGroup& m)
    {
        if (m.held || m.jobs > 0 || m.freed) return;
        m.freed = true;
        for (size_t s = 0; s < m.slots.size(); s++) drop_merged(m, s);
        for (int c : m.ctx) ctxs[(size_t)c].held = false;
    }
    void destroy(const Handle& h)
    {
        if (h.type == CTX) {
            spf_destroy(ctxs[(size_t)h.idx].h);
            ctxs[(size_t)h.idx].held = false;
            step = "spf_destroy";
        } else if (h.type == GROUP) {
            MGroup& m = groups[(size_t)h.idx];
            spf_group_destroy(m.h);
            m.held = false;
            maybe_free(m);
            step = "spf_group_destroy";
        } else {
            MGraph& g = graphs[(size_t)h.idx];
            spf_graph_destroy(g.h);
            g.alive = false;
            ctxs[(size_t)g.ctx].kids--;
            if (g.grp >= 0) {
                MGroup& m = groups[(size_t)g.grp];
                for (size_t s = 0; s < m.slots.size(); s++) // the merged graph that held this job goes with it
                    if (std::find(m.slots[s].jobs.begin(), m.slots[s].jobs.end(), h.idx) != m.slots[s].jobs.end()) drop_merged(m, s);
                m.jobs--;
                maybe_free(m);
            }
            step = "spf_graph_destroy";
        }
        check();
    }
    // the handles in the order given (indices into `handles`), then: nothing may be left
    bool take_apart(const std::vector<size_t>& order)
    {
        for (size_t k : order) destroy(handles[k]); // (to the end after a mismatch too: the order is what is under test)
        spf_live_counts got;
        if (ok && (spf_live_objects(&got) != SPF_OK || got.contexts || got.groups || got.graphs || got.pools || got.values)) {
            fprintf(stderr, "lifetimes: handles are left after the last destroy\n");
            ok = false;
        }
        return ok;
    }
};

struct LifetimeScenario {
    const char* name;
    std::function<bool(const spf_params&)> run;
};

std::vector<LifetimeScenario> lifetime_scenarios()
{
    std::vector<LifetimeScenario> v;
    v.push_back({"context, graph: graph first", [](const spf_params& p) { Forest f(p); f.add_graph(f.add_ctx()); return f.take_apart({1, 0}); }});
    v.push_back({"context, graph: context first", [](const spf_params& p) { Forest f(p); f.add_graph(f.add_ctx()); return f.take_apart({0, 1}); }});
    v.push_back({"group, job: job first", [](const spf_params& p) { Forest f(p); f.add_job(f.add_group(1)); return f.take_apart({1, 0}); }});
    v.push_back({"group, job: group first", [](const spf_params& p) { Forest f(p); f.add_job(f.add_group(1)); return f.take_apart({0, 1}); }});
    static const size_t perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    static const char* const perm_names[6] = {"group, two jobs: group, job 0, job 1", "group, two jobs: group, job 1, job 0", "group, two jobs: job 0, group, job 1",
                                              "group, two jobs: job 0, job 1, group", "group, two jobs: job 1, group, job 0", "group, two jobs: job 1, job 0, group"};
    for (int k = 0; k < 6; k++)
        v.push_back({perm_names[k], [k](const spf_params& p) {
                         Forest f(p);
                         const int g = f.add_group(2);
                         f.add_job(g);
                         f.add_job(g);
                         return f.take_apart({perms[k][0], perms[k][1], perms[k][2]});
                     }});
    // two jobs filed under merged[1], whose merged graph was made by spf_graph_create on member 1's context
    auto merged = [](const spf_params& p, std::vector<size_t> order) {
        Forest f(p);
        const int g = f.add_group(2);
        f.add_job(g, 1);
        f.add_job(g, 1);
        f.file_merged();
        return f.take_apart(order);
    };
    v.push_back({"merged entry: its job first", [merged](const spf_params& p) { return merged(p, {1, 2, 0}); }});
    v.push_back({"merged entry: the group first", [merged](const spf_params& p) { return merged(p, {0, 1, 2}); }});
    v.push_back({"merged entry: the other job of the entry first", [merged](const spf_params& p) { return merged(p, {2, 0, 1}); }});
    v.push_back({"borrowed member context: graph, then group, then graph", [](const spf_params& p) {
                     Forest f(p);
                     const int g = f.add_group(2);
                     f.add_borrowed_graph(g, 1);
                     f.add_borrowed_graph(g, 1);
                     return f.take_apart({1, 0, 2});
                 }});
    return v;
}

// a seeded random forest, taken apart in a uniformly random order
bool random_forest(const spf_params& p, Rng& r)
{
    Forest f(p);
    const int n_ctx = 1 + (int)r.below(3), n_grp = (int)r.below(3);
    for (int i = 0; i < n_ctx; i++) f.add_ctx();
    for (int i = 0; i < n_grp; i++) f.add_group(1 + (int)r.below(3));
    for (int i = 0; i < n_ctx; i++)
        for (size_t k = r.below(7); k > 0; k--) f.add_graph(i, r.below(12));
    for (int i = 0; i < n_grp; i++) {
        const int members = (int)f.groups[(size_t)i].ctx.size();
        for (size_t k = r.below(7); k > 0; k--) switch (r.below(3)) {
            case 0: f.add_job(i, -1, r.below(12)); break;
            case 1: f.add_job(i, (int)r.below((size_t)members), r.below(12)); break; // filed under a merged entry
            default: f.add_borrowed_graph(i, (int)r.below((size_t)members), r.below(12)); break;
            }
    }
    f.file_merged();
    std::vector<size_t> order(f.handles.size());
    for (size_t k = 0; k < order.size(); k++) order[k] = k;
    for (size_t k = order.size(); k > 1; k--) std::swap(order[k - 1], order[r.below(k)]); // Fisher-Yates
    return f.take_apart(order);
}

} // namespace

int main(int argc, char** argv)
{
    if (argc > 1 && (!strncmp(argv[1], "--lifetimes", 11) || !strcmp(argv[1], "--selftest-lifetime"))) {
        spf_params tiny;
        spf_default_params(&tiny);
        tiny.lwe_dimension = 2; tiny.polynomial_degree = 16; tiny.ks_radix_count = 2; tiny.tr_radix_count = 2; tiny.ss_radix_count = 2;
        tiny.pbs_radix_log = 4; tiny.cbs_radix_count = 2;
        if (!strcmp(argv[1], "--selftest-lifetime")) {
            // the sanitizer sees this class of error: a group freed with a bare `delete`, past its reference count, and then its job
            // destroyed — the run must die with a heap-use-after-free report in group_forget_graph (tests/test_lifetimes_host.py)
            Forest f(tiny);
            const int g = f.add_group(1);
            const int job = f.add_job(g);
            delete f.groups[(size_t)g].h;
            spf_graph_destroy(f.graphs[(size_t)job].h);
            printf("selftest: no report?!\n");
            return 0;
        }
        if (!strcmp(argv[1], "--lifetimes")) { // --lifetimes [scenario index]: every scenario, or the one named
            const std::vector<LifetimeScenario> all = lifetime_scenarios();
            const long only = argc > 2 ? strtol(argv[2], nullptr, 10) : -1;
            size_t done = 0;
            for (size_t k = 0; k < all.size(); k++) {
                if (only >= 0 && (size_t)only != k) continue;
                const bool good = all[k].run(tiny);
                printf("lifetimes %2zu: %s: %s\n", k, all[k].name, good ? "ok" : "MISMATCH");
                fflush(stdout);
                if (!good) return 1;
                done++;
            }
            printf("lifetimes: %zu scenarios, live counts as the model after every step, nothing left, no sanitizer report\n", done);
            return done ? 0 : 2;
        }
        if (!strcmp(argv[1], "--lifetimes-random")) { // --lifetimes-random <cases> <seed>
            const uint64_t cases = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1000;
            Rng r(argc > 3 ? strtoull(argv[3], nullptr, 10) : 0x11FE71E5);
            uint64_t destroyed = 0;
            for (uint64_t it = 0; it < cases; it++) {
                if (!random_forest(tiny, r)) { fprintf(stderr, "lifetimes-random: case %" PRIu64 " failed\n", it); return 1; }
                destroyed++;
            }
            printf("lifetimes-random: %" PRIu64 " forests taken apart in random order, live counts as the model after every step, no sanitizer report\n", destroyed);
            return 0;
        }
        fprintf(stderr, "unknown mode %s\n", argv[1]);
        return 2;
    }
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
    spf_params k2 = tiny; // a generic set with glwe_size 2 (and a cbs count that is no power of two)
    k2.glwe_size = 2; k2.polynomial_degree = 64; k2.cbs_radix_count = 3;
    if (!batch_shapes_match_the_header(dflt) || !batch_shapes_match_the_header(k2) || !batch_shapes_match_the_header(tiny)) return 1;
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
                    st = spf_graph_add_op(g, (spf_graph_op)r.below(16), r.below(10) ? in : nullptr, r.below(5), r.below(2) ? r() : r.below(5000), &node);
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
                if (n.op >= 70 && n.op <= 72) { // SPF_OP_GLWE_KEYSWITCH / _AUTOMORPHISM / _TRACE: the nodes of their named constructors
                    if (n.n_in != 1 || n.kind != SPF_VAL_GLWE1) { fprintf(stderr, "graph: bad node accepted\n"); return 1; }
                    if (n.in[0] >= i || g->nodes[n.in[0]].kind != SPF_VAL_GLWE1) { fprintf(stderr, "graph: bad operand accepted\n"); return 1; }
                    if (n.op == 70 ? n.param >= SPF_GLWE_KSK_SLOTS : n.op == 71 ? (n.param < 1 || n.param > 11) : n.param != 0) { fprintf(stderr, "graph: bad parameter accepted\n"); return 1; }
                    continue;
                }
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
