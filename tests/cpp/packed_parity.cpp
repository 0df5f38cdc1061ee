// Native parity test of the packed-integer methods of `Evaluation` (include/spf_evaluation.hpp) — test infrastructure.
// Unpacks a batch of packed GLWEs to L1 LWEs and to GGSWs, and packs a batch of bit GLWEs; the expectation is the CPU
// oracle's composition of the reference's steps: `SampleExtract(i)` for every bit
// (fluent/packed_dynamic_generic_int_graph_node.rs:24-39), then `KeyswitchL1toL0` -> `CircuitBootstrap`
// (fhe_circuit.rs:563-625); `MulXN(i)` of bit i summed (fluent/dynamic_generic_int_graph_nodes.rs:139-200).  Links
// libspf_hip.so (product) and libspf_oracle.so (checker); built and run by tests/test_gpu_packed.py.
#include "spf_evaluation.hpp"

extern "C" {
#include "spf_oracle.h"
}

#include <cstdio>
#include <cstring>
#include <vector>

namespace {

int failures = 0;
void expect(bool ok, const char* what)
{
    std::printf("%-58s %s\n", what, ok ? "ok" : "MISMATCH");
    if (!ok) failures++;
}
template <class T> bool same(const std::vector<T>& a, const std::vector<T>& b)
{
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}

} // namespace

int main()
{
    spf_params p;
    spf_default_params(&p);
    p.lwe_dimension = 10; // a short blind rotation keeps the oracle quick; every other parameter is DEFAULT_128
    const size_t n = p.lwe_dimension, N = p.polynomial_degree, k = p.glwe_size;
    const double lwe_std = 7.25e-5, glwe_std = 7e-16;
    const size_t ggsw_pbs = (k + 1) * p.pbs_radix_count * (k + 1) * (N / 2);
    size_t logn = 0;
    while (((size_t)1 << logn) < N) logn++;
    const size_t ak_len = logn * k * p.tr_radix_count * (k + 1) * (N / 2);
    const size_t ssk_len = (k * (k + 1) / 2) * p.ss_radix_count * (k + 1) * (N / 2);
    const size_t cbs_len = (k + 1) * p.cbs_radix_count * (k + 1) * (N / 2);

    spfo_rng r;
    spfo_rng_seed(&r, 0x9AC3);
    std::vector<uint64_t> lwe_sk(n), glwe_sk(k * N);
    spfo_gen_binary_key(&r, lwe_sk.data(), n);
    spfo_gen_binary_key(&r, glwe_sk.data(), k * N);
    std::vector<spfo_c64> bsk(n * ggsw_pbs), ak(ak_len), ssk(ssk_len);
    spfo_gen_bsk_fft(&r, bsk.data(), lwe_sk.data(), n, glwe_sk.data(), N, k, p.pbs_radix_log, p.pbs_radix_count, glwe_std);
    std::vector<uint64_t> ksk(k * N * p.ks_radix_count * (n + 1));
    spfo_gen_ksk(&r, ksk.data(), glwe_sk.data(), k * N, lwe_sk.data(), n, p.ks_radix_log, p.ks_radix_count, lwe_std);
    spfo_gen_auto_key_fft(&r, ak.data(), glwe_sk.data(), N, k, p.tr_radix_log, p.tr_radix_count, glwe_std);
    spfo_gen_ssk_fft(&r, ssk.data(), glwe_sk.data(), N, k, p.ss_radix_log, p.ss_radix_count, glwe_std);

    const size_t B = 3, bits = 5, gw = (k + 1) * N, lw = k * N + 1;
    std::vector<uint64_t> packed(B * gw), bit_glwe(B * bits * gw);
    for (auto& x : packed) x = spfo_rng_next(&r);
    for (auto& x : bit_glwe) x = spfo_rng_next(&r);

    // the oracle: every row of the unpack, its GGSW, and the pack as MulXN(i) + GlweAdd
    std::vector<uint64_t> lwe_ref(B * bits * lw), l0(n + 1), pack_ref(B * gw, 0), shifted(gw), acc(gw);
    std::vector<double> ggsw_ref(B * bits * cbs_len * 2);
    for (size_t b = 0; b < B; b++)
        for (size_t i = 0; i < bits; i++) {
            uint64_t* row = lwe_ref.data() + (b * bits + i) * lw;
            spfo_sample_extract(row, packed.data() + b * gw, i, N, k);
            if (i < 2) { // the circuit bootstrap of two rows per ciphertext; the GPU's others are held to its own keyswitch + CBS
                spfo_keyswitch_lwe(l0.data(), row, ksk.data(), k * N, n, p.ks_radix_log, p.ks_radix_count);
                spfo_circuit_bootstrap(reinterpret_cast<spfo_c64*>(ggsw_ref.data()) + (b * bits + i) * cbs_len, l0.data(), bsk.data(),
                                       ak.data(), ssk.data(), n, N, k, p.pbs_radix_log, p.pbs_radix_count, p.tr_radix_log,
                                       p.tr_radix_count, p.ss_radix_log, p.ss_radix_count, p.cbs_radix_log, p.cbs_radix_count);
            }
        }
    for (size_t b = 0; b < B; b++) {
        std::memcpy(acc.data(), bit_glwe.data() + b * bits * gw, gw * 8);
        for (size_t i = 1; i < bits; i++) {
            spfo_glwe_mul_xn(shifted.data(), bit_glwe.data() + (b * bits + i) * gw, i, N, k);
            spfo_glwe_xor(acc.data(), acc.data(), shifted.data(), N, k);
        }
        std::memcpy(pack_ref.data() + b * gw, acc.data(), gw * 8);
    }

    try {
        spf::ComputeKey key{reinterpret_cast<const double*>(bsk.data()), bsk.size(), ksk.data(), ksk.size(),
                            reinterpret_cast<const double*>(ak.data()), ak.size(), reinterpret_cast<const double*>(ssk.data()), ssk.size()};
        spf::Evaluation ev(key, p, 0);
        std::vector<uint64_t> lwe(B * bits * lw), out(B * gw);
        ev.unpack_l1(lwe.data(), packed.data(), bits, B);
        expect(same(lwe, lwe_ref), "Evaluation::unpack_l1 (B = 3, 5 bits)");
        std::vector<double> ggsw(B * bits * cbs_len * 2), ggsw_ks(B * bits * cbs_len * 2);
        ev.unpack_circuit_bootstrap(ggsw.data(), packed.data(), bits, B);
        bool oracle_rows = true;
        for (size_t b = 0; b < B; b++)
            for (size_t i = 0; i < 2; i++) {
                const size_t o = (b * bits + i) * cbs_len * 2;
                oracle_rows &= std::memcmp(ggsw.data() + o, ggsw_ref.data() + o, cbs_len * 16) == 0;
            }
        expect(oracle_rows, "Evaluation::unpack_circuit_bootstrap, rows 0-1 vs the oracle");
        spf_status st = spf_group_keyswitch_circuit_bootstrap_batch(ev.group(), B * bits, lwe.data(), ggsw_ks.data());
        expect(st == SPF_OK && same(ggsw, ggsw_ks), "  ... every row == keyswitch_circuit_bootstrap of the LWEs");
        ev.pack(out.data(), bit_glwe.data(), bits, B);
        expect(same(out, pack_ref), "Evaluation::pack (B = 3, 5 bits)");
        std::vector<uint64_t> one(gw);
        ev.pack(one.data(), bit_glwe.data() + 2 * bits * gw, bits);
        expect(same(one, std::vector<uint64_t>(pack_ref.begin() + 2 * gw, pack_ref.end())), "  ... one ciphertext");
        bool threw = false;
        try { ev.unpack_l1(lwe.data(), packed.data(), N + 1, 1); } catch (const spf::Error& e) { threw = e.status == SPF_ERR_INVALID_ARGUMENT; }
        expect(threw, "  ... n_bits = N + 1 throws");
    } catch (const spf::Error& e) {
        std::printf("spf::Error: %s\n", e.what());
        return 2;
    }
    std::printf("%s\n", failures ? "FAILED" : "all equal");
    return failures ? 1 : 0;
}
